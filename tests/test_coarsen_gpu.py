"""A map coarsened 2:1 into a map of twice the voxel size on the GPU (include/tsdf_hip_coarsen.h)
against tests/coarsenref.py, bit for bit: export_bricks() of the destination as uint32, the set of
brick coordinates included (an empty brick left behind fails), and the seven counts of the
contract.  tsdf_coarsen_count runs before tsdf_coarsen_into and must leave both maps unchanged.
The reference works on the source's exported bricks and never sees the library's lists.  Source
maps are one scan cropped to a box of bricks, so the numpy reference is instant; the uncropped map
at 5 cm, whose parent bricks outnumber the per-brick kernels' grid cap, is coarsened once."""
import ctypes as C

import numpy as np
import pytest

import coarsenref as cr
import oracle
import sampleref as sr

pytestmark = pytest.mark.gpu

F = np.float32
VS, TAU = sr.VOXEL_SIZE, sr.SDF_TRUNC
VS2 = 2.0 * VS
SMALL = dict(max_bricks=1 << 14, max_points=1 << 17, max_batch=4)
CROP = ((6, -11, -7), (15, -2, 2))  # brick coordinates, as tests/test_merge_gpu.py crops
# (bricks, voxels, parent bricks, coarse voxels by number of valid children n = 1..8 at
# min_weight 0 and at 2): the CPU oracle's map of the same crop
CROP_COUNTS = {
    "vdbfusion_f64": (65, 8293, 23, [16, 11, 18, 1443, 74, 66, 65, 151],
                      [5, 15, 17, 1520, 63, 66, 43, 103]),
    "voxblox": (63, 7347, 23, [32, 149, 71, 1259, 98, 94, 46, 49],
                [77, 267, 163, 1028, 32, 43, 28, 23]),
}
SEMS = ["vdbfusion_f64", "voxblox"]
COARSEN_GRID_CAP = 4096  # tsdf_coarsen.hip (tests/test_coarsen_plan.py reads it there)
LIM = 1 << 20


def hip(sem="vdbfusion_f64", vs=VS, tau=TAU, **kw):
    from tsdf_map import HipTSDFVolume
    return HipTSDFVolume(vs, tau, semantics=sem, **dict(SMALL, **kw))


def text(v):
    return v._lib.tsdf_last_error(v._ctx).decode()


def raw_call(dst, src, box=None, side=0, min_children=1, min_weight=0.0, count=False, stats=True):
    """The C entry points through ctypes: (rc, counts).  box: (lo, hi), either may be None."""
    from tsdf_map import _abi
    fn = dst._lib.tsdf_coarsen_count if count else dst._lib.tsdf_coarsen_into
    st = _abi.CoarsenStats(9, 9, 9, 9, 9, 9, 9)
    lo, hi = (None, None) if box is None else box
    plo = None if lo is None else (C.c_int32 * 3)(*lo)
    phi = None if hi is None else (C.c_int32 * 3)(*hi)
    rc = fn(dst._ctx, None if src is None else src._ctx, plo, phi, side, min_children, min_weight,
            C.byref(st) if stats else None)
    return rc, st.as_dict()


def coarsen_and_check(dst, src, min_children=1, min_weight=0.0, box=None, side="inside",
                      src_bricks=None):
    """tsdf_coarsen_count, then tsdf_coarsen_into, both against the reference; returns
    (Expected, the call's counts)."""
    before = dst.export_bricks()
    src_before = src.export_bricks() if src_bricks is None else src_bricks
    exp = cr.expected(dst, src, min_children, min_weight, box, side, dst_bricks=before,
                      src_bricks=src_before)
    dry = dst.coarsen_from(src, min_children, min_weight, box=box, side=side, dry_run=True)
    assert dry == exp.counts, (dry, exp.counts)
    cr.assert_same_bricks(dst.export_bricks(), before)  # the count changed nothing
    cr.assert_same_bricks(src.export_bricks(), src_before)
    st = dst.coarsen_from(src, min_children, min_weight, box=box, side=side)
    assert st == dry
    cr.assert_same_bricks(dst.export_bricks(), exp)
    cr.assert_same_bricks(src.export_bricks(), src_before)  # src is never modified
    return exp, st


def tiny(voxels, sdf, weight, sem="vdbfusion_f64", vs=VS):
    v = hip(sem, vs=vs)
    v.import_bricks(*cr.bricks_of(voxels, sdf, weight, cr.background(v)))
    return v


@pytest.fixture(scope="module")
def maps(scan0):
    """Per semantics: the scan-0 map at 10 cm cropped to CROP with its exports, and the export of
    the scan-0 map at 20 cm.  The full scan in vdbfusion_f64, every second point in voxblox."""
    pts, org = scan0
    out = {}
    for sem, p in (("vdbfusion_f64", pts), ("voxblox", np.ascontiguousarray(pts[::2]))):
        v = hip(sem)
        v.integrate(p, org)
        v.sync()
        n = v.num_bricks()
        gone = v.evict_outside(*CROP, copy_out=False)
        assert 0 < gone == n - v.num_bricks()
        c = hip(sem, vs=VS2)
        c.integrate(p, org)
        c.sync()
        out[sem] = dict(crop=v, voxels=v.export_voxels(), bricks=v.export_bricks(),
                        full20=c.export_bricks())
        c.close()
    yield out
    for m in out.values():
        m["crop"].close()


def test_the_crops_are_what_the_issue_counted(maps):
    for sem, (nb, nv, npar, h0, h2) in CROP_COUNTS.items():
        m = maps[sem]
        assert m["crop"].num_bricks() == nb and m["voxels"][0].shape[0] == nv
        assert cr.coarsen(cr.empty_bricks(), m["bricks"], 0.0).counts["parent_bricks"] == npar
        # every class of child count is populated: no case of the matrix is vacuous
        assert cr.child_histogram(m["bricks"], 0.0) == h0
        assert cr.child_histogram(m["bricks"], 2.0) == h2
        assert min(h0 + h2) >= 5
        print(sem, "20 cm map:", m["full20"][0].shape[0], "bricks")


@pytest.mark.parametrize("into", ["empty", "scan0"])
@pytest.mark.parametrize("min_weight", [0.0, 2.0])
@pytest.mark.parametrize("min_children", [1, 4, 8])
@pytest.mark.parametrize("sem", SEMS)
def test_bitwise_matrix(maps, sem, min_children, min_weight, into):
    m = maps[sem]
    hist = CROP_COUNTS[sem][3 if min_weight == 0.0 else 4]
    dst = hip(sem, vs=VS2)
    if into == "scan0":
        dst.import_bricks(*m["full20"])
    exp, st = coarsen_and_check(dst, m["crop"], min_children, min_weight, src_bricks=m["bricks"])
    print("%s mc %d mw %g into %s: %s" % (sem, min_children, min_weight, into, st))
    assert st["src_bricks"] == CROP_COUNTS[sem][0] and st["parent_bricks"] == CROP_COUNTS[sem][2]
    assert st["coarse_voxels"] == sum(hist[min_children - 1:]) >= 20
    assert st["child_voxels"] == sum((k + 1) * h for k, h in enumerate(hist) if k + 1 >= min_children)
    assert st["parent_bricks"] >= st["touched_bricks"] >= st["new_bricks"]
    if into == "empty":
        assert st["overlap_voxels"] == 0
        assert st["new_bricks"] == st["touched_bricks"] == dst.num_bricks() > 0
    else:  # the same scan at 20 cm observed most of these voxels: both fuse branches occur
        assert 0 < st["overlap_voxels"] <= st["coarse_voxels"]
        assert st["new_bricks"] < st["touched_bricks"]
    dst.close()


# ---- tiny adversarial maps -----------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEMS)
def test_a_single_voxel_at_each_child_position(sem):
    V = np.array([3, -5, 7])
    for k in range(8):
        src = tiny([2 * V + [k & 1, (k >> 1) & 1, k >> 2]], [0.07], [4.0], sem)
        dst = hip(sem, vs=VS2)
        exp, st = coarsen_and_check(dst, src)
        assert exp.voxels.tolist() == [V.tolist()]
        assert st == dict(src_bricks=1, parent_bricks=1, touched_bricks=1, new_bricks=1,
                          coarse_voxels=1, overlap_voxels=0, child_voxels=1)
        ijk, s, w = dst.export_voxels()
        assert ijk.tolist() == [V.tolist()] and w[0] == F(4.0)
        assert s[0] == F(F(F(0.07) * F(4.0)) / F(4.0))
        # a second time: the voxel is held now (rule 6's mean), and min_children = 2 takes nothing
        _, st = coarsen_and_check(dst, src)
        assert st["overlap_voxels"] == 1 and st["new_bricks"] == 0
        _, st = coarsen_and_check(dst, src, min_children=2)
        assert st["touched_bricks"] == 0 and st["parent_bricks"] == 1
        src.close()
        dst.close()


def test_the_corner_of_eight_source_bricks():
    """The voxels 7 and 8 per axis: eight source bricks, eight coarse voxels (3 and 4 per axis) of
    one destination brick, each with one child from its own source brick."""
    v = np.array([[7 + dx, 7 + dy, 7 + dz] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
    src = tiny(v, np.linspace(-0.2, 0.2, 8), np.arange(1, 9))
    assert src.num_bricks() == 8
    dst = hip(vs=VS2)
    exp, st = coarsen_and_check(dst, src)
    assert st == dict(src_bricks=8, parent_bricks=1, touched_bricks=1, new_bricks=1,
                      coarse_voxels=8, overlap_voxels=0, child_voxels=8)
    assert dst.export_bricks()[0].tolist() == [[0, 0, 0]]
    for mw, n in ((1.5, 7), (8.0, 1), (8.5, 0)):
        d2 = hip(vs=VS2)
        _, st = coarsen_and_check(d2, src, min_weight=mw)
        assert st["coarse_voxels"] == n and d2.num_bricks() == (1 if n else 0)
        d2.close()
    src.close()
    dst.close()


def test_the_eight_bricks_of_one_parent():
    D = np.array([-3, 2, -1])
    v = [8 * (2 * D + [j & 1, (j >> 1) & 1, j >> 2]) + [2 * (j % 4), 5, 3] for j in range(8)]
    src = tiny(v, np.linspace(-0.1, 0.25, 8), np.arange(1, 9))
    assert src.num_bricks() == 8
    dst = hip(vs=VS2)
    exp, st = coarsen_and_check(dst, src)
    assert st == dict(src_bricks=8, parent_bricks=1, touched_bricks=1, new_bricks=1,
                      coarse_voxels=8, overlap_voxels=0, child_voxels=8)
    assert dst.export_bricks()[0].tolist() == [D.tolist()]
    # a box that selects four of them: the other four read as unobserved
    box = ((-6, 4, -2), (-5, 6, 0))
    d2 = hip(vs=VS2)
    _, st = coarsen_and_check(d2, src, box=box)
    assert st["src_bricks"] == 4 and st["coarse_voxels"] == 4 and st["parent_bricks"] == 1
    _, st = coarsen_and_check(d2, src, box=box, side="outside")
    assert st["src_bricks"] == 4 and st["new_bricks"] == 0 and st["overlap_voxels"] == 0
    cr.assert_same_bricks(d2.export_bricks(), dst.export_bricks())
    for x in (src, dst, d2):
        x.close()


@pytest.mark.parametrize("sem", SEMS)
def test_bricks_at_negative_odd_coordinates(sem):
    rng = np.random.default_rng(3)
    # ((-1, -1, -1) and (-2, -1, -1) share the parent (-1, -1, -1): five parents)
    bricks = np.array([[-1, -1, -1], [-3, -5, -7], [-1, 0, 1], [-7, 3, -1], [1, -3, 5], [-2, -1, -1]])
    assert np.unique(bricks >> 1, axis=0).shape[0] == 5
    c = bricks[np.argsort(cr._brick_key(bricks))].astype(np.int32)
    w = rng.integers(0, 4, (len(c), 8, 8, 8)).astype(F)
    s = rng.uniform(-TAU, TAU, w.shape).astype(F)
    src = hip(sem)
    s[w == 0] = cr.background(src)
    src.import_bricks(c, s, w)
    for mc, mw in ((1, 0.0), (3, 0.0), (5, 2.0), (8, 1.0)):
        dst = hip(sem, vs=VS2)
        exp, st = coarsen_and_check(dst, src, mc, mw)
        assert st["src_bricks"] == 6 and st["parent_bricks"] == 5
        assert st["coarse_voxels"] > 0 and exp.coords.min() < 0
        dst.close()
    src.close()


def test_a_brick_below_min_weight_leaves_nothing_behind():
    v = [[0, 0, 0], [1, 0, 0], [40, 40, 40], [41, 41, 41]]
    src = tiny(v, [0.1, 0.1, 0.2, 0.2], [1.0, 1.5, 3.0, 4.0])
    dst = hip(vs=VS2)
    exp, st = coarsen_and_check(dst, src, min_weight=2.0)
    assert st["src_bricks"] == 2 and st["parent_bricks"] == 2
    assert st["touched_bricks"] == st["new_bricks"] == 1 < st["parent_bricks"]
    assert dst.export_bricks()[0].tolist() == [[2, 2, 2]]
    d2 = hip(vs=VS2)
    _, st = coarsen_and_check(d2, src, min_weight=5.0)
    assert st["touched_bricks"] == 0 and st["parent_bricks"] == 2 and d2.num_bricks() == 0
    for x in (src, dst, d2):
        x.close()


def test_pool_order_does_not_show(maps):
    """The same field in two pool orders -- imported in (z, y, x) order, and in reverse behind a
    decoy whose eviction moves the pool's last brick into slot 0 -- coarsens to the same bits."""
    c, s, w = maps["vdbfusion_f64"]["bricks"]
    a, b = hip(), hip()
    a.import_bricks(c, s, w)
    decoy = np.array([[500, 500, 500]], np.int32)
    b.import_bricks(decoy, s[:1], w[:1])
    b.import_bricks(c[::-1], s[::-1], w[::-1])
    assert b.evict_outside((-400, -400, -400), (400, 400, 400), copy_out=False) == 1
    cr.assert_same_bricks(b.export_bricks(), (c, s, w))
    out = []
    for src in (a, b):
        dst = hip(vs=VS2)
        dst.import_bricks(*[x[::3] for x in maps["vdbfusion_f64"]["full20"]])
        coarsen_and_check(dst, src, 2, 0.0, src_bricks=(c, s, w))
        out.append(dst.export_bricks())
        dst.close()
    cr.assert_same_bricks(out[0], out[1])
    a.close()
    b.close()


def test_the_ends_of_the_packable_range():
    v = [[8 * -LIM, 8 * -LIM + 1, 8 * -LIM + 7], [8 * (LIM - 1) + 7, 8 * (LIM - 1) + 6, 8 * (LIM - 1)],
         [8 * -LIM + 6, 8 * (LIM - 1) + 7, 3]]
    src = tiny(v, [0.1, -0.1, 0.05], [1.0, 2.0, 3.0])
    assert src.export_bricks()[0].min() == -LIM and src.export_bricks()[0].max() == LIM - 1
    dst = hip(vs=VS2)
    exp, st = coarsen_and_check(dst, src)
    assert st["parent_bricks"] == st["new_bricks"] == 3 and st["coarse_voxels"] == 3
    c = dst.export_bricks()[0]
    assert c.min() == -(LIM >> 1) and c.max() == (LIM >> 1) - 1
    assert sorted(map(tuple, exp.voxels.tolist())) == sorted(
        tuple(x >> 1 for x in p) for p in v)
    # a box that ends at the range's ends selects them; one short of them does not
    d2 = hip(vs=VS2)
    _, st = coarsen_and_check(d2, src, box=((-LIM, -LIM, -LIM), (LIM, LIM, LIM)))
    assert st["src_bricks"] == 3
    _, st = coarsen_and_check(d2, src, box=((-LIM + 1, -LIM, -LIM), (LIM - 1, LIM, LIM)))
    assert st["src_bricks"] == 0 and st["parent_bricks"] == 0
    for x in (src, dst, d2):
        x.close()


def test_an_empty_source_and_an_empty_selection(maps):
    dst, src = hip(vs=VS2), hip()
    dst.import_bricks(*cr.bricks_of([[1, 2, 3]], [0.1], [2.0], F(TAU)))
    before = dst.export_bricks()
    for dry in (True, False):
        st = dst.coarsen_from(src, dry_run=dry)
        assert not any(st.values()), st
        st = dst.coarsen_from(maps["vdbfusion_f64"]["crop"], box=((0, 0, 0), (0, 9, 9)), dry_run=dry)
        assert not any(st.values()), st
        st = dst.coarsen_from(maps["vdbfusion_f64"]["crop"], box=CROP, side="outside", dry_run=dry)
        assert not any(st.values()), st
    cr.assert_same_bricks(dst.export_bricks(), before)
    dst.close()
    src.close()


# ---- rule 9 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("into", ["empty", "scan0"])
@pytest.mark.parametrize("sem", SEMS)
def test_inside_then_outside_equals_the_whole(maps, sem, into):
    m = maps[sem]
    box = ((8, -9, -5), (13, -4, 0))  # odd and even faces: parents straddle the box
    whole, parts = hip(sem, vs=VS2), hip(sem, vs=VS2)
    if into == "scan0":
        for d in (whole, parts):
            d.import_bricks(*m["full20"])
    _, sw = coarsen_and_check(whole, m["crop"], 2, 0.0, src_bricks=m["bricks"])
    _, si = coarsen_and_check(parts, m["crop"], 2, 0.0, box, "inside", src_bricks=m["bricks"])
    _, so = coarsen_and_check(parts, m["crop"], 2, 0.0, box, "outside", src_bricks=m["bricks"])
    cr.assert_same_bricks(parts.export_bricks(), whole.export_bricks())
    assert si["src_bricks"] > 0 and so["src_bricks"] > 0
    for k in ("src_bricks", "coarse_voxels", "child_voxels", "overlap_voxels"):
        assert si[k] + so[k] == sw[k], k
    assert si["parent_bricks"] + so["parent_bricks"] > sw["parent_bricks"]  # shared parents
    assert si["coarse_voxels"] >= 20 and so["coarse_voxels"] >= 20
    whole.close()
    parts.close()


# ---- more parent bricks than the grid cap --------------------------------------------------------

def test_past_the_grid_cap(scan0):
    """k_coarsen_flag and k_coarsen_apply take one parent brick per workgroup, 4096 workgroups at
    the most: scan 0 at 5 cm has more parents than that, into an empty map and then once more into
    the result (every brick held, every voxel an overlap)."""
    pts, org = scan0
    src = hip(vs=0.05, tau=0.15, max_bricks=1 << 16)
    src.integrate(pts, org)
    src.sync()
    bricks = src.export_bricks()
    dst = hip(vs=0.1, tau=0.15, max_bricks=1 << 14)
    exp = cr.expected(dst, src, src_bricks=bricks)
    print("5 cm: %d bricks, %s" % (bricks[0].shape[0], exp.counts))
    assert exp.counts["parent_bricks"] > COARSEN_GRID_CAP
    assert exp.counts["coarse_voxels"] >= 100000
    # (by hand, not coarsen_and_check: the 120 MB source is read back once, at the end)
    assert dst.coarsen_from(src, dry_run=True) == exp.counts
    assert dst.num_bricks() == 0
    st = dst.coarsen_from(src)
    assert st == exp.counts and st["new_bricks"] == st["touched_bricks"] == dst.num_bricks()
    cr.assert_same_bricks(dst.export_bricks(), exp)
    exp2 = cr.coarsen(exp[:3], bricks, cr.background(dst), min_children=3)
    st = dst.coarsen_from(src, min_children=3)
    assert st == exp2.counts
    assert st["new_bricks"] == 0 and st["overlap_voxels"] == st["coarse_voxels"] > 10000
    cr.assert_same_bricks(dst.export_bricks(), exp2)
    cr.assert_same_bricks(src.export_bricks(), bricks)
    src.close()
    dst.close()


# ---- capacity ------------------------------------------------------------------------------------

def held_elsewhere(m, n):
    """n bricks of the 20 cm map that are no parent of the crop."""
    c, s, w = m["full20"]
    par = cr._brick_key(np.asarray(m["bricks"][0], np.int64) >> 1)
    keep = np.nonzero(~np.isin(cr._brick_key(c), par))[0][:n]
    assert keep.size == n
    return c[keep], s[keep], w[keep]


def test_growth(maps):
    m = maps["vdbfusion_f64"]
    dst = hip(vs=VS2, max_bricks=64)
    dst.import_bricks(*held_elsewhere(m, 50))
    g0 = dst.stats()["n_grows"]
    exp, st = coarsen_and_check(dst, m["crop"], src_bricks=m["bricks"])
    assert 50 + st["new_bricks"] > 64
    after = dst.stats()
    assert after["n_grows"] > g0 and after["max_bricks"] >= after["n_bricks"] == 50 + st["new_bricks"]
    dst.close()


def test_no_room_leaves_both_maps_alone(maps):
    from tsdf_map import TsdfError, _abi
    m = maps["vdbfusion_f64"]
    dst = hip(vs=VS2, max_bricks=64, max_bricks_hard=64)
    dst.import_bricks(*held_elsewhere(m, 50))
    before = dst.export_bricks()
    exp = cr.expected(dst, m["crop"], dst_bricks=before, src_bricks=m["bricks"])
    assert 50 + exp.counts["new_bricks"] > 64
    with pytest.raises(TsdfError) as e:
        dst.coarsen_from(m["crop"])
    assert e.value.code == _abi.TSDF_ENOMEM and "do not fit" in str(e.value)
    assert e.value.stats == exp.counts  # the counts are filled
    cr.assert_same_bricks(dst.export_bricks(), before)
    cr.assert_same_bricks(m["crop"].export_bricks(), m["bricks"])
    assert dst.stats()["n_grows"] == 0
    # a call that fits still works afterwards
    small = tiny([[5, -3, 9]], [0.07], [4.0])
    coarsen_and_check(dst, small)
    for v in (dst, small):
        v.close()


# ---- refusals ------------------------------------------------------------------------------------

def test_refusals(maps):
    from tsdf_map import _abi
    m = maps["vdbfusion_f64"]
    src = m["crop"]
    dst = hip(vs=VS2)
    dst.import_bricks(*[a[:5] for a in m["full20"]])
    before = dst.export_bricks()
    E = _abi.TSDF_EINVAL
    lo, hi = CROP

    def refused(rc_st, msg, code=E, d=dst):
        assert rc_st[0] == code and text(d) == msg, (rc_st, text(d))

    for count in (False, True):
        refused(raw_call(dst, None, count=count), "coarsen: the source context is NULL")
        refused(raw_call(dst, dst, count=count),
                "coarsen: source and destination are the same context")
        for side in (-1, 2, 7):
            refused(raw_call(dst, src, side=side, count=count),
                    "coarsen: side must be TSDF_COARSEN_INSIDE or _OUTSIDE")
        for box in ((lo, None), (None, hi)):
            refused(raw_call(dst, src, box=box, count=count),
                    "coarsen: exactly one of lo and hi is NULL")
        for mc in (0, 9, 0xFFFFFFFF):
            refused(raw_call(dst, src, min_children=mc, count=count),
                    "coarsen: min_children must be 1..8")
        for mw in (-1.0, float("nan"), -1e-30):
            refused(raw_call(dst, src, min_weight=mw, count=count),
                    "coarsen: min_weight is negative or NaN")
    refused(raw_call(dst, src, count=True, stats=False), "coarsen: null argument")
    # the first broken rule is the one reported
    refused(raw_call(dst, src, box=(lo, None), side=9, min_children=0, min_weight=-1.0),
            "coarsen: side must be TSDF_COARSEN_INSIDE or _OUTSIDE")
    refused(raw_call(dst, src, box=(lo, None), min_children=0, min_weight=-1.0),
            "coarsen: exactly one of lo and hi is NULL")
    refused(raw_call(dst, src, min_children=0, min_weight=-1.0),
            "coarsen: min_children must be 1..8")
    # contexts that do not go together
    twice = "coarsen: the destination's voxel size is not twice the source's"
    for other, msg in ((hip(vs=VS, tau=TAU), twice), (hip(vs=0.4, tau=TAU), twice),
                       (hip(vs=float(np.nextafter(F(VS2), F(1))), tau=TAU), twice),
                       (hip(vs=VS2, tau=0.2), "coarsen: the contexts' truncation distances differ"),
                       (hip("voxblox", vs=VS2),
                        "coarsen: the contexts' backgrounds differ (Voxblox against VDBFusion)")):
        refused(raw_call(other, src), msg, d=other)
        other.close()
    refused(raw_call(src, dst), twice, d=src)  # the other way round is no coarsening
    shard = hip(vs=VS2, n_sectors=2, sector=0)
    refused(raw_call(shard, src),
            "coarsen: the destination context holds one sector shard of the map (n_sectors > 1); "
            "coarsening a sharded field is not supported", d=shard)
    shard.close()
    shard = hip(n_sectors=2, sector=0)
    refused(raw_call(dst, shard),
            "coarsen: the source context holds one sector shard of the map (n_sectors > 1); "
            "coarsening a sharded field is not supported")
    shard.close()
    # every refusal left both maps as they were, and the stats untouched
    assert raw_call(dst, None)[1] == dict.fromkeys(raw_call(dst, None)[1], 9)
    cr.assert_same_bricks(dst.export_bricks(), before)
    cr.assert_same_bricks(src.export_bricks(), m["bricks"])
    # vdbfusion and vdbfusion_f64 share field format and background: they may be mixed
    f32 = hip("vdbfusion", vs=VS2)
    rc, st = raw_call(f32, src)
    assert rc == _abi.TSDF_OK and st["coarse_voxels"] == sum(CROP_COUNTS["vdbfusion_f64"][3]), text(f32)
    cr.assert_same_bricks(f32.export_bricks(),
                          cr.coarsen(cr.empty_bricks(), m["bricks"], F(TAU)))
    # NULL stats are fine for the call itself; a box with lo > hi is an empty box
    rc, _ = raw_call(dst, src, stats=False)
    assert rc == _abi.TSDF_OK, text(dst)
    rc, st = raw_call(dst, src, box=((5, 5, 5), (1, 9, 9)))
    assert rc == _abi.TSDF_OK and not any(st.values())
    f32.close()
    dst.close()


def test_an_open_border_reduce_is_refused():
    import torch
    from tsdf_map import _abi
    a, b, src = hip(vs=VS2), hip(vs=VS2), hip()
    for v in (a, b, src):
        v.import_bricks(*cr.bricks_of([[1, 2, 3]], [0.1], [2.0], F(TAU)))
    fine = hip()
    fine.import_bricks(*cr.bricks_of([[2, 4, 6]], [0.1], [2.0], F(TAU)))
    dev = torch.device("cuda", 0)
    allk = torch.full((2, 1), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for r, v in enumerate((a, b)):
        assert v.brick_keys_into(allk[r].data_ptr(), 1) == 1
    send = torch.empty((1, 1028), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    counts, sent = np.array([1, 1], np.uint64), np.zeros(2, np.uint64)
    rc = b._lib.tsdf_border_pack_device(b._ctx, C.c_void_p(allk.data_ptr()),
                                        counts.ctypes.data_as(_abi.U64P), 1, 2, 1,
                                        C.c_void_p(send.data_ptr()), 1,
                                        sent.ctypes.data_as(_abi.U64P))
    assert rc == _abi.TSDF_OK and sent.tolist() == [1, 0], text(b)
    rc, _ = raw_call(b, src)
    assert rc == _abi.TSDF_EINVAL and text(b) == (
        "coarsen: a border reduce is open on the destination context: commit or abort it first "
        "(tsdf_border_commit_device)")
    coarse4 = hip(vs=2 * VS2)
    rc, _ = raw_call(coarse4, b)
    assert rc == _abi.TSDF_EINVAL and text(coarse4) == (
        "coarsen: a border reduce is open on the source context: commit or abort it first "
        "(tsdf_border_commit_device)")
    b.border_commit(False)
    rc, st = raw_call(b, fine)  # fine voxel (2, 4, 6) is a child of b's voxel (1, 2, 3)
    assert rc == _abi.TSDF_OK and st["overlap_voxels"] == 1, text(b)
    for v in (a, b, src, fine, coarse4):
        v.close()


def test_contexts_on_different_devices_are_refused():
    import torch
    from tsdf_map import _abi
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    a, b = hip(vs=VS2, device_id=0), hip(device_id=1)
    rc, _ = raw_call(a, b)
    assert rc == _abi.TSDF_EINVAL and text(a) == \
        "coarsen: the contexts are on different devices (0 and 1)"
    a.close()
    b.close()


# ---- the coarsened map is a map like any other ---------------------------------------------------

@pytest.mark.parametrize("pipeline", [0, 2])
def test_a_scan_integrated_after_the_coarsening_is_the_reference_routes(maps, sim, pipeline):
    m = maps["vdbfusion_f64"]
    dst = hip(vs=VS2, pipeline=pipeline)
    dst.import_bricks(*[a[::2] for a in m["full20"]])
    exp = cr.expected(dst, m["crop"], 2, 0.0, src_bricks=m["bricks"])
    st = dst.coarsen_from(m["crop"], 2)
    assert st == exp.counts and st["new_bricks"] > 0 and st["overlap_voxels"] > 0
    # the reference route: the expected bricks imported into fresh volumes, the same scan
    twin = oracle.OracleTSDFVolume(VS2, TAU)
    twin.import_bricks(*exp[:3])
    route = hip(vs=VS2, pipeline=pipeline)
    route.import_bricks(*exp[:3])
    pts, org = sim.scan(1)
    pts = np.ascontiguousarray(pts[::4])
    for v in (dst, twin, route):
        v.integrate(pts, org)
    got = dst.export_bricks()
    cr.assert_same_bricks(got, twin.export_bricks())
    cr.assert_same_bricks(got, route.export_bricks())
    for v in (dst, twin, route):
        v.close()


def test_queries_read_the_coarsened_field(maps, scan0):
    """sample, raycast, the indexed mesh, esdf and column_map on the coarsened volume against the
    same calls on a volume that got the expected bricks through import_bricks."""
    m = maps["vdbfusion_f64"]
    dst = hip(vs=VS2)
    dst.import_bricks(*m["full20"])
    exp = cr.expected(dst, m["crop"], src_bricks=m["bricks"])
    st = dst.coarsen_from(m["crop"])
    assert st["overlap_voxels"] >= 1000  # the field the queries read has changed
    twin = hip(vs=VS2)
    twin.import_bricks(*exp[:3])
    pts, org = scan0
    q = np.ascontiguousarray(pts[::16]).astype(F)
    c = exp.voxels
    lo, hi = c.min(0) - 2, c.max(0) + 3
    n_valid = {}
    for mode in ("nearest", "trilinear"):
        a, b = dst.sample(q, mode=mode), twin.sample(q, mode=mode)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
        n_valid[mode] = int(a[3].sum())
    assert n_valid["nearest"] >= 100
    d = (q - org.astype(F))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    a, b = dst.raycast(org, d, t_max=30.0), twin.raycast(org, d, t_max=30.0)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    assert int(a[2].sum()) >= 100
    a, b = dst.extract_indexed_mesh(), twin.extract_indexed_mesh()
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    assert a[1].shape[0] >= 100
    a, b = dst.esdf(lo, hi, 1.0), twin.esdf(lo, hi, 1.0)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    a, b = dst.column_map(lo, hi), twin.column_map(lo, hi)
    for k in ("elev", "ceil", "n_occ", "n_free", "flags"):
        assert np.array_equal(getattr(a, k).view(np.uint8), getattr(b, k).view(np.uint8)), k
    assert int((a.n_occ > 0).sum()) >= 10
    dst.close()
    twin.close()


# ---- the Python layer ----------------------------------------------------------------------------

def test_coarsened_and_the_pyramid(maps):
    from tsdf_map import lod_pyramid
    m = maps["vdbfusion_f64"]
    src = m["crop"]
    one = src.coarsened()
    assert one.semantics == src.semantics and one.voxel_size == 2.0 * src.voxel_size
    assert one.sdf_trunc == src.sdf_trunc and one.params.max_bricks == src.params.max_bricks
    e1 = cr.coarsen(cr.empty_bricks(), m["bricks"], F(TAU))
    cr.assert_same_bricks(one.export_bricks(), e1)
    levels = lod_pyramid(src, 3, min_children=2, min_weight=0.0)
    assert len(levels) == 4 and levels[0] is src
    assert [v.voxel_size for v in levels] == [VS, 2 * VS, 4 * VS, 8 * VS]
    ref = m["bricks"]
    for v in levels[1:]:
        ref = cr.coarsen(cr.empty_bricks(), ref, F(TAU), min_children=2)[:3]
        cr.assert_same_bricks(v.export_bricks(), ref)
    assert 0 < levels[3].num_bricks() < levels[2].num_bricks() < levels[1].num_bricks()
    cr.assert_same_bricks(src.export_bricks(), m["bricks"])
    assert lod_pyramid(src, 0) == [src]
    with pytest.raises(ValueError):
        lod_pyramid(src, -1)
    with pytest.raises(ValueError):
        src.coarsened(min_children=9)
    with pytest.raises(ValueError):
        one.coarsen_from(src, side="around")
    for v in levels[1:] + [one]:
        v.close()


def test_a_sliding_window_keeps_a_coarse_map_of_what_left(scan0):
    from tsdf_map import SlidingWindow
    pts, org = scan0
    p = np.ascontiguousarray(pts[::2])
    live, plain, whole = hip(), hip(), hip()
    coarse = hip(vs=VS2)
    win = SlidingWindow(live, 3.0, every=1000, coarse=coarse)
    ref = SlidingWindow(plain, 3.0, every=1000)
    whole.integrate(p, org)
    whole.sync()
    for w in (win, ref):
        w.integrate(p, org)
        n1 = w.evict(org)
        assert 0 < n1 < whole.num_bricks() and w.volume.num_bricks() > 0
        w.radius_m = 0.0
        n2 = w.evict(org + np.array([1e4, 1e4, 1e4]))
        assert n2 > 0 and w.volume.num_bricks() == 0 and n1 + n2 == whole.num_bricks()
    # no brick left twice: the coarse map is the coarsening of the un-evicted map, bit for bit
    want = whole.coarsened()
    cr.assert_same_bricks(coarse.export_bricks(), want.export_bricks())
    cr.assert_same_bricks(coarse.export_bricks(),
                          cr.coarsen(cr.empty_bricks(), whole.export_bricks(), F(TAU)))
    # and the archive is what it is without `coarse`
    assert len(win.archive) == len(ref.archive) == 2
    for a, b in zip(win.archive, ref.archive):
        cr.assert_same_bricks(a, b)
    with pytest.raises(ValueError):
        SlidingWindow(live, 3.0, coarse=hip_closing(VS))
    for v in (live, plain, whole, coarse, want):
        v.close()


def hip_closing(vs):
    """A volume for a constructor that refuses it (closed by its finaliser)."""
    return hip(vs=vs)
