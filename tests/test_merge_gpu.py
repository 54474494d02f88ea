"""One map merged into another under a rigid transform on the GPU (include/tsdf_hip_merge.h) against
tests/mergeref.py, bit for bit: export_bricks() of the destination as uint32, the set of brick
coordinates included (an empty brick left behind fails), and the four counts of the contract.  The
reference enumerates the destination voxels generously and never sees the library's candidate
list.  Source maps are one scan cropped to a box of bricks, so the numpy reference is instant; the
uncropped map, whose candidates outnumber the per-brick kernels' grid cap, is merged in four cases
(tests/pastcap.py)."""
import ctypes as C

import numpy as np
import pytest

import mergeref as mr
import oracle
import pastcap as pc
import sampleref as sr

pytestmark = pytest.mark.gpu

F = np.float32
VS, TAU = sr.VOXEL_SIZE, sr.SDF_TRUNC
SMALL = dict(max_bricks=1 << 14, max_points=1 << 17, max_batch=4)
CROP = ((6, -11, -7), (15, -2, 2))  # brick coordinates
CROP_COUNTS = {"vdbfusion_f64": (65, 8293), "voxblox": (63, 7347)}
SEMS = ["vdbfusion_f64", "voxblox"]
MODES = ["nearest", "trilinear"]
POSES = {
    "identity": mr.rigid(),
    "half_voxel": mr.rigid(t=(0.05, 0.05, 0.05)),
    "z90": mr.rot_z90((1.0, 2.0, 0.3)),
    "general": mr.rigid((10.0, -20.0, 30.0), (1.234, -2.345, 0.456)),
}


def hip(sem="vdbfusion_f64", vs=VS, tau=TAU, **kw):
    from tsdf_map import HipTSDFVolume
    return HipTSDFVolume(vs, tau, semantics=sem, **dict(SMALL, **kw))


def text(v):
    return v._lib.tsdf_last_error(v._ctx).decode()


def raw_call(dst, src, pose, mode=1, min_weight=0.0, count=False, stats=True):
    """The C entry points through ctypes: (rc, counts or None)."""
    from tsdf_map import _abi
    fn = dst._lib.tsdf_merge_count if count else dst._lib.tsdf_merge_transformed
    st = _abi.MergeStats(9, 9, 9, 9, 9, 9)
    p = None if pose is None else (C.c_double * 12)(*np.asarray(pose, np.float64).reshape(12))
    rc = fn(dst._ctx, None if src is None else src._ctx, p, mode, min_weight,
            C.byref(st) if stats else None)
    return rc, st.as_dict()


def bricks_of(voxels, sdf, weight, bg):
    v = np.asarray(voxels, np.int64).reshape(-1, 3)
    b, inv = np.unique(v >> 3, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    S = np.full((b.shape[0], 8, 8, 8), F(bg), F)
    W = np.zeros((b.shape[0], 8, 8, 8), F)
    S[inv, v[:, 2] & 7, v[:, 1] & 7, v[:, 0] & 7] = np.asarray(sdf, F)
    W[inv, v[:, 2] & 7, v[:, 1] & 7, v[:, 0] & 7] = np.asarray(weight, F)
    return b.astype(np.int32), S, W


def merge_and_check(dst, src, pose, mode, min_weight=0.0, reach=1, src_voxels=None):
    """tsdf_merge_count, then tsdf_merge_transformed, both against the reference; returns
    (Expected, the call's counts)."""
    before = dst.export_bricks()
    src_before = src.export_bricks()
    exp = mr.expected(dst, src, pose, mode, min_weight, reach, src_voxels=src_voxels,
                      dst_bricks=before)
    dry = dst.merge_from(src, pose, mode=mode, min_weight=min_weight, dry_run=True)
    assert mr.contract_counts(dry) == exp.counts, (dry, exp.counts)
    mr.assert_same_bricks(dst.export_bricks(), before)  # the count changed nothing
    st = dst.merge_from(src, pose, mode=mode, min_weight=min_weight)
    assert st == dry
    assert st["src_bricks"] == src_before[0].shape[0]
    assert st["candidate_bricks"] >= st["touched_bricks"] >= st["new_bricks"]
    mr.assert_same_bricks(dst.export_bricks(), exp)
    mr.assert_same_bricks(src.export_bricks(), src_before)  # src is never modified
    return exp, st


@pytest.fixture(scope="module")
def maps(scan0):
    """Per semantics: the uncropped scan-0 map's export, and the map cropped to CROP with its
    exports.  The full scan in vdbfusion_f64, every second point in voxblox."""
    pts, org = scan0
    out = {}
    for sem, p in (("vdbfusion_f64", pts), ("voxblox", np.ascontiguousarray(pts[::2]))):
        v = hip(sem)
        v.integrate(p, org)
        v.sync()
        full = v.export_bricks()
        n = v.num_bricks()
        gone = v.evict_outside(*CROP, copy_out=False)
        assert 0 < gone == n - v.num_bricks()
        out[sem] = dict(crop=v, full=full, voxels=v.export_voxels(), bricks=v.export_bricks())
    yield out
    for m in out.values():
        m["crop"].close()


def test_the_crops_are_what_the_issue_counted(maps):
    for sem, (nb, nv) in CROP_COUNTS.items():
        assert maps[sem]["crop"].num_bricks() == nb
        assert maps[sem]["voxels"][0].shape[0] == nv
        print(sem, "uncropped:", maps[sem]["full"][0].shape[0], "bricks")


@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("into", ["empty", "scan0"])
@pytest.mark.parametrize("min_weight", [0.0, 2.0])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sem", SEMS)
def test_bitwise_matrix(maps, sem, mode, min_weight, into, pose):
    m = maps[sem]
    dst = hip(sem)
    if into == "scan0":
        dst.import_bricks(*m["full"])
    exp, st = merge_and_check(dst, m["crop"], POSES[pose], mode, min_weight,
                              src_voxels=m["voxels"])
    print("%s %s mw %g into %s, %s: %s" % (sem, mode, min_weight, into, pose, st))
    # not vacuous, asserted on the reference
    floor = 50 if (pose == "z90" and mode == "trilinear") else 1000
    assert exp.counts["merged_voxels"] >= floor, exp.counts
    if into == "scan0":
        # both fuse branches occur: the crop lies inside the map it is merged into under the
        # identity and the half-voxel shift; the quarter turn lands it across the map's rim, on
        # held bricks and new ones; the general pose lands it in free space
        if pose in ("identity", "half_voxel"):
            assert exp.counts["overlap_voxels"] >= 1000 and exp.counts["new_bricks"] == 0
        elif pose == "z90" and mode == "nearest":
            assert 100 <= exp.counts["overlap_voxels"] < exp.counts["merged_voxels"]
            assert 0 < exp.counts["new_bricks"] < exp.counts["touched_bricks"]
    else:
        assert exp.counts["overlap_voxels"] == 0
        assert exp.counts["new_bricks"] == exp.counts["touched_bricks"] == dst.num_bricks()
    if pose == "general" and mode == "nearest" and into == "empty" and min_weight == 0.0:
        assert exp.counts["new_bricks"] > m["crop"].num_bricks()  # e.g. 112 against 65
    if pose == "identity" and mode == "nearest" and into == "empty" and min_weight == 0.0:
        mr.assert_same_bricks(dst.export_bricks(), m["bricks"])  # an exact copy
    dst.close()


def test_an_empty_source():
    dst, src = hip(), hip()
    dst.import_bricks(*bricks_of([[1, 2, 3]], [0.1], [2.0], F(TAU)))
    before = dst.export_bricks()
    for dry in (True, False):
        st = dst.merge_from(src, POSES["general"], dry_run=dry)
        assert not any(st.values()), st
    mr.assert_same_bricks(dst.export_bricks(), before)
    # the other way round: into an empty map, and an image wholly outside the index domain
    st = src.merge_from(dst, POSES["identity"], mode="nearest")
    assert st == dict(src_bricks=1, candidate_bricks=st["candidate_bricks"], touched_bricks=1,
                      new_bricks=1, merged_voxels=1, overlap_voxels=0)
    far = hip()
    st = far.merge_from(dst, mr.rigid(t=(1e6, 0.0, 0.0)), mode="nearest")
    assert st["src_bricks"] == 1 and st["touched_bricks"] == 0 and far.num_bricks() == 0
    for v in (dst, src, far):
        v.close()


def test_an_image_far_outside_the_domain_is_an_empty_merge(maps):
    """Finite poses that put the image outside the index domain on one axis or on all: out there
    the search pad is as wide as the domain, and the candidate box must still be empty (a loop over
    the other two axes would not end).  Zero counts at once, and nothing changed."""
    import time
    m = maps["vdbfusion_f64"]
    dst = hip()
    dst.import_bricks(*[a[:5] for a in m["full"]])
    before = dst.export_bricks()
    t0 = time.perf_counter()
    for mag in (8.4e5, 1e12, 1e38):
        for axes in ((1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 1)):
            T = mr.rigid((10.0, -20.0, 30.0), tuple(mag * a for a in axes))
            for mode in MODES:
                for dry in (True, False):
                    st = dst.merge_from(m["crop"], T, mode=mode, dry_run=dry)
                    assert st == dict(src_bricks=65, candidate_bricks=0, touched_bricks=0,
                                      new_bricks=0, merged_voxels=0, overlap_voxels=0), (mag, axes, st)
    assert time.perf_counter() - t0 < 5.0
    # a translation whose inverse leaves the fp32 range is refused like a non-finite entry
    from tsdf_map import _abi
    rc, _ = raw_call(dst, m["crop"], mr.rigid((10.0, -20.0, 30.0), (3e38, 3e38, 3e38)))
    assert rc == _abi.TSDF_EINVAL and text(dst) == "merge: pose is NULL or has a non-finite entry"
    mr.assert_same_bricks(dst.export_bricks(), before)
    dst.close()


@pytest.mark.parametrize("mode", MODES)
def test_one_observed_voxel(mode):
    src = hip()
    src.import_bricks(*bricks_of([[5, -3, 9]], [0.07], [4.0], F(TAU)))
    for name, T in list(POSES.items()) + [("two_voxels", mr.rigid(t=(0.2, 0.0, -0.1)))]:
        dst = hip()
        exp, st = merge_and_check(dst, src, T, mode)
        if mode == "trilinear":
            assert st["merged_voxels"] == 0 and dst.num_bricks() == 0  # nothing allocated
        elif name in ("identity", "two_voxels"):
            assert st["merged_voxels"] == 1 and dst.num_bricks() == 1
        dst.close()
    src.close()


@pytest.mark.parametrize("sem", SEMS)
def test_the_cube_across_a_brick_corner(sem):
    v = np.array([[7 + dx, 7 + dy, 7 + dz] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
    src = hip(sem)
    src.import_bricks(*bricks_of(v, np.linspace(-0.2, 0.2, 8), np.arange(1, 9), mr.background(src)))
    assert src.num_bricks() == 8
    merged = {}
    for name, T in POSES.items():
        for mode in MODES:
            for mw in (0.0, 1.5):
                dst = hip(sem)
                _, st = merge_and_check(dst, src, T, mode, mw)
                merged[(name, mode, mw)] = st["merged_voxels"]
                dst.close()
    assert merged[("identity", "nearest", 0.0)] == 8 and merged[("identity", "nearest", 1.5)] == 7
    assert merged[("half_voxel", "trilinear", 0.0)] == 1  # the cube's centre
    assert merged[("half_voxel", "trilinear", 1.5)] == 0  # every corner must pass
    src.close()


def test_pool_order_does_not_show(maps):
    """The same field in two pool orders -- imported in (z, y, x) order, and with a brick moved
    into a hole from the pool's last slot by an evict -- merges to the same bits."""
    c, s, w = maps["vdbfusion_f64"]["bricks"]
    a, b = hip(), hip()
    a.import_bricks(c, s, w)
    # b: the bricks in reverse order and a decoy first, then the decoy evicted: the brick at the
    # pool's last slot fills slot 0
    decoy = np.array([[500, 500, 500]], np.int32)
    b.import_bricks(decoy, s[:1], w[:1])
    b.import_bricks(c[::-1], s[::-1], w[::-1])
    assert b.evict_outside((-400, -400, -400), (400, 400, 400), copy_out=False) == 1
    mr.assert_same_bricks(b.export_bricks(), (c, s, w))
    out = []
    for src in (a, b):
        for mode in MODES:
            dst = hip()
            merge_and_check(dst, src, POSES["general"], mode, src_voxels=maps["vdbfusion_f64"]["voxels"])
            out.append(dst.export_bricks())
            dst.close()
    mr.assert_same_bricks(out[0], out[2])
    mr.assert_same_bricks(out[1], out[3])
    a.close()
    b.close()


def test_the_same_merge_twice_gives_the_same_bits(maps):
    m = maps["voxblox"]
    out = []
    for _ in range(2):
        dst = hip("voxblox")
        dst.import_bricks(*m["full"])
        dst.merge_from(m["crop"], POSES["general"], mode="trilinear")
        out.append(dst.export_bricks())
        dst.close()
    mr.assert_same_bricks(out[0], out[1])


# ---- the index domain's edge and far coordinates -------------------------------------------------

EDGE_VS, EDGE_TAU = 0.05, 0.15
LIM = 1 << 23


@pytest.fixture(scope="module")
def edge_map(sim):
    """The geometry of test_domain_edge.py: scan 0 (every 16th point) with its origin 3 m inside
    the +x edge of the index domain and 2 m inside the -y edge, at 5 cm; cropped to the bricks
    within 12 bricks of the +x edge so that the reference stays small.  A single sparse scan at
    5 cm has no fully observed cube out there, so four solid bricks in the domain's corner give
    the trilinear mode something to merge."""
    pts, org = sim.scan(0)
    L = LIM * EDGE_VS
    sh = np.array([L - 3.0 - org[0], -(L - 2.0) - org[1], 0.0])
    p = np.ascontiguousarray((pts[::16].astype(np.float64) + sh).astype(F))
    v = hip(vs=EDGE_VS, tau=EDGE_TAU)
    v.integrate(p, org + sh)
    v.sync()
    top = 1 << 20
    v.evict_outside((top - 12, -top, -top), (top, top, top), copy_out=False)
    rng = np.random.default_rng(5)
    solid = np.array([[top - 2 + i, -top + j, 40] for j in (0, 1) for i in (0, 1)], np.int32)
    v.import_bricks(solid, rng.uniform(-EDGE_TAU, EDGE_TAU, (4, 8, 8, 8)).astype(F),
                    rng.integers(1, 9, (4, 8, 8, 8)).astype(F))
    vox = v.export_voxels()
    assert 100 <= v.num_bricks() <= 400 and vox[0][:, 0].max() == LIM - 1
    yield v, vox
    v.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shift", ["identity", "one_voxel_out", "one_voxel_in"])
def test_at_the_edge_of_the_index_domain(edge_map, mode, shift):
    """Under the identity the map is resampled where it is; one voxel further out, the part that
    would pass |i| < 2^23 is dropped and the rest is bitwise.  fp32 coordinates are 0.6 voxels
    apart out there, so the reference enumerates with reach 3."""
    src, vox = edge_map
    T = mr.rigid(t=({"identity": 0.0, "one_voxel_out": EDGE_VS, "one_voxel_in": -EDGE_VS}[shift],
                    0.0, 0.0))
    dst = hip(vs=EDGE_VS, tau=EDGE_TAU)
    exp, st = merge_and_check(dst, src, T, mode, reach=3, src_voxels=vox)
    print("edge %s %s: %s" % (shift, mode, st))
    c, _, w = dst.export_bricks()
    assert np.all((c >= -(1 << 20)) & (c < (1 << 20)))
    assert st["merged_voxels"] >= (1000 if mode == "nearest" else 100)
    hi = exp.voxels[:, 0].max()
    if mode == "nearest":  # right up to the last voxel of the domain
        assert hi == LIM - 1 if shift != "one_voxel_in" else hi >= LIM - 4
    else:  # inside the solid bricks, the 16 voxels below the edge
        assert LIM - 16 <= hi <= LIM - 1
    dst.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_translation_of_4_km(maps, mode):
    """4 km at 10 cm: coordinates of 4 * 10^4 voxels, where the search pad is 20 times what it is
    at the origin (merge_plan.h).  Out and back again."""
    m = maps["vdbfusion_f64"]
    T = mr.rigid((10.0, -20.0, 30.0), (4000.0, -4000.0, 12.3))
    far = hip()
    exp, st = merge_and_check(far, m["crop"], T, mode, src_voxels=m["voxels"])
    assert st["merged_voxels"] >= 1000 and np.abs(exp.voxels).max() > 39000
    if mode == "nearest":
        back = hip()
        exp2, st2 = merge_and_check(back, far, mr.invert(T), mode)
        assert st2["merged_voxels"] >= 1000 and np.abs(exp2.voxels).max() < 400
        back.close()
    far.close()


# ---- capacity ------------------------------------------------------------------------------------

def test_growth(maps):
    m = maps["vdbfusion_f64"]
    dst = hip(max_bricks=64)
    dst.import_bricks(*[a[:40] for a in m["full"]])
    g0 = dst.stats()["n_grows"]
    exp, st = merge_and_check(dst, m["crop"], POSES["general"], "nearest", src_voxels=m["voxels"])
    assert 40 + st["new_bricks"] > 64
    after = dst.stats()
    assert after["n_grows"] > g0 and after["max_bricks"] >= after["n_bricks"] == 40 + st["new_bricks"]
    dst.close()


def test_no_room_leaves_both_maps_alone(maps):
    from tsdf_map import TsdfError, _abi
    m = maps["vdbfusion_f64"]
    dst = hip(max_bricks=64, max_bricks_hard=64)
    dst.import_bricks(*[a[:40] for a in m["full"]])
    before = dst.export_bricks()
    exp = mr.expected(dst, m["crop"], POSES["general"], "nearest", src_voxels=m["voxels"],
                      dst_bricks=before)
    assert 40 + exp.counts["new_bricks"] > 64
    with pytest.raises(TsdfError) as e:
        dst.merge_from(m["crop"], POSES["general"], mode="nearest")
    assert e.value.code == _abi.TSDF_ENOMEM and "do not fit" in str(e.value)
    assert mr.contract_counts(e.value.stats) == exp.counts  # the counts are filled
    mr.assert_same_bricks(dst.export_bricks(), before)
    mr.assert_same_bricks(m["crop"].export_bricks(), m["bricks"])
    assert dst.stats()["n_grows"] == 0
    # a merge that fits still works afterwards
    small = hip()
    small.import_bricks(*bricks_of([[5, -3, 9]], [0.07], [4.0], F(TAU)))
    merge_and_check(dst, small, POSES["identity"], "nearest")
    for v in (dst, small):
        v.close()


# ---- against the parent's route, GPU against GPU -------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_equals_sample_then_import_on_the_uncropped_map(maps, mode):
    """export -> host enumeration -> tsdf_sample -> tsdf_import_bricks, what a caller had to do
    before: the same field, with no numpy sampling in between."""
    m = maps["vdbfusion_f64"]
    src = hip()
    src.import_bricks(*m["full"])
    T = POSES["general"]
    ijk = src.export_voxels()[0]
    v = mr.candidate_voxels(ijk, T, VS)
    q = mr.preimage(mr.inverse_pose(T), v, VS)
    s, w, _, valid = src.sample(q, mode=mode, min_weight=0.0)
    assert valid.sum() >= 10000
    route = hip()
    route.import_bricks(*bricks_of(v[valid], s[valid], w[valid], F(TAU)))
    dst = hip()
    st = dst.merge_from(src, T, mode=mode)
    assert st["candidate_bricks"] > pc.MERGE_CAP
    assert st["merged_voxels"] == int(valid.sum()) and st["new_bricks"] == route.num_bricks()
    mr.assert_same_bricks(dst.export_bricks(), route.export_bricks())
    for x in (src, route, dst):
        x.close()


# ---- more candidate bricks than the grid cap, against the numpy reference ------------------------

@pytest.fixture(scope="module")
def full_source(maps):
    """The uncropped scan-0 map as a volume (8693 bricks) and its export_voxels()."""
    src = hip()
    src.import_bricks(*maps["vdbfusion_f64"]["full"])
    yield src, src.export_voxels()
    src.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(pc.MERGE_CASES))
def test_past_the_grid_cap(maps, full_source, case, mode):
    """k_merge_flag and k_merge_apply take one candidate brick per workgroup, 8192 workgroups at
    the most.  Into an empty map under the general pose; and into a map that holds every second
    brick of the source under the half-voxel shift, where held and new candidates alternate and
    the slot a workgroup hands round in LDS changes from trip to trip."""
    full = maps["vdbfusion_f64"]["full"]
    src, voxels = full_source
    pose = pc.MERGE_CASES[case][0]
    assert np.array_equal(pose, POSES["general" if case == "empty_general" else "half_voxel"])
    dst = hip(max_bricks=1 << 15)
    held = pc.merge_destination(full, case)
    if held[0].shape[0]:
        dst.import_bricks(*held)
    exp, st = merge_and_check(dst, src, pose, mode, src_voxels=voxels)
    print("%s %s: %s" % (case, mode, st))
    # the candidate list is what tests/test_merge_plan.py's restated search lists
    assert st["candidate_bricks"] == pc.merge_candidates(full[0], pose, mode) > pc.MERGE_CAP
    pc.assert_merge_past_cap(case, st["candidate_bricks"], exp.counts)
    dst.close()


# ---- the merged map is a map like any other ------------------------------------------------------

@pytest.mark.parametrize("pipeline", [0, 2])
def test_a_scan_integrated_after_the_merge_is_the_oracles(maps, sim, pipeline):
    m = maps["vdbfusion_f64"]
    dst = hip(pipeline=pipeline)
    dst.import_bricks(*[a[::2] for a in m["full"]])
    dst.merge_from(m["crop"], POSES["half_voxel"], mode="trilinear")
    twin = oracle.OracleTSDFVolume(VS, TAU)
    twin.import_bricks(*dst.export_bricks())
    pts, org = sim.scan(1)
    pts = np.ascontiguousarray(pts[::4])
    dst.integrate(pts, org)
    twin.integrate(pts, org)
    mr.assert_same_bricks(dst.export_bricks(), twin.export_bricks())
    dst.close()
    twin.close()


def test_queries_read_the_merged_field(maps, scan0):
    """sample, raycast, esdf and both meshes after a merge, each against its own reference run on
    the merged map's export."""
    from test_prune_gpu import cut_box
    from test_queries_after_change_gpu import Refs, check
    m = maps["vdbfusion_f64"]
    dst = hip()
    dst.import_bricks(*m["full"])
    before = sr.field_of(dst)
    st = dst.merge_from(m["crop"], POSES["half_voxel"], mode="nearest")  # into held bricks
    assert st["overlap_voxels"] >= 1000 and st["new_bricks"] == 0
    st = dst.merge_from(m["crop"], POSES["z90"], mode="nearest")         # and new ones beside them
    assert st["overlap_voxels"] >= 100 and st["new_bricks"] >= 10
    twin = oracle.OracleTSDFVolume(VS, TAU)
    twin.import_bricks(*dst.export_bricks())
    c = dst.export_bricks()[0]
    refs = Refs(dst, cut_box(c), (sr.jitter_queries(*scan0), scan0))
    # the change shows in the queries: some samples differ from the map before the merge
    s0 = sr.sample(before, refs.queries, sr.TRILINEAR)[0]
    assert (refs.get("sample", "trilinear")[0] != s0).sum() >= 100
    check(dst, refs, twin, kinds=("sample", "raycast", "esdf", "mesh", "imesh"))
    dst.close()
    twin.close()


# ---- refusals ------------------------------------------------------------------------------------

def test_refusals(maps):
    from tsdf_map import _abi
    m = maps["vdbfusion_f64"]
    src = m["crop"]
    dst = hip()
    dst.import_bricks(*[a[:5] for a in m["full"]])
    before = dst.export_bricks()
    eye, E = POSES["identity"], _abi.TSDF_EINVAL

    def refused(rc_st, msg, code=E, d=dst):
        assert rc_st[0] == code and text(d) == msg, (rc_st, text(d))

    for count in (False, True):
        refused(raw_call(dst, None, eye, count=count), "merge: the source context is NULL")
        refused(raw_call(dst, dst, eye, count=count),
                "merge: source and destination are the same context")
        for mode in (-1, 2, 7):
            refused(raw_call(dst, src, eye, mode=mode, count=count),
                    "merge: mode must be TSDF_SAMPLE_NEAREST or _TRILINEAR")
        for mw in (-1.0, float("nan"), -1e-30):
            refused(raw_call(dst, src, eye, min_weight=mw, count=count),
                    "merge: min_weight is negative or NaN")
        refused(raw_call(dst, src, None, count=count), "merge: pose is NULL or has a non-finite entry")
        for k, bad in ((0, np.nan), (3, np.inf), (11, -np.inf), (6, np.nan)):
            T = POSES["general"].copy()
            T.reshape(12)[k] = bad
            refused(raw_call(dst, src, T, count=count),
                    "merge: pose is NULL or has a non-finite entry")
        rot = "merge: pose is not a rigid transform (max |R R^T - I| > 1e-5 or det <= 0)"
        for T in (np.diag([1.0, 1.0, -1.0, 1.0])[:3], np.diag([1.00002, 1.0, 1.0, 1.0])[:3],
                  np.zeros((3, 4)), POSES["general"] * 2.0):
            refused(raw_call(dst, src, T, count=count), rot)
    refused(raw_call(dst, src, eye, count=True, stats=False), "merge: null argument")
    # the first broken rule is the one reported
    refused(raw_call(dst, src, None, mode=9, min_weight=-1.0),
            "merge: mode must be TSDF_SAMPLE_NEAREST or _TRILINEAR")
    # contexts that do not go together
    for other, msg in ((hip(vs=0.05, tau=TAU), "merge: the contexts' voxel sizes differ"),
                       (hip(vs=VS, tau=0.2), "merge: the contexts' truncation distances differ"),
                       (hip("voxblox"), "merge: the contexts' backgrounds differ (Voxblox against "
                                        "VDBFusion)")):
        refused(raw_call(dst, other, eye), msg)
        refused(raw_call(other, dst, eye), msg, d=other)
        other.close()
    shard = hip(n_sectors=2, sector=0)
    refused(raw_call(dst, shard, eye),
            "merge: the source context holds one sector shard of the map (n_sectors > 1); merging a "
            "sharded field is not supported")
    refused(raw_call(shard, dst, eye),
            "merge: the destination context holds one sector shard of the map (n_sectors > 1); "
            "merging a sharded field is not supported", d=shard)
    shard.close()
    # every refusal left both maps as they were, and the stats untouched
    assert raw_call(dst, None, eye)[1] == dict.fromkeys(raw_call(dst, None, eye)[1], 9)
    mr.assert_same_bricks(dst.export_bricks(), before)
    mr.assert_same_bricks(src.export_bricks(), m["bricks"])
    # vdbfusion and vdbfusion_f64 share field format and background: they may be mixed
    f32 = hip("vdbfusion")
    rc, st = raw_call(f32, src, eye, mode=0)
    assert rc == _abi.TSDF_OK and st["merged_voxels"] == m["voxels"][0].shape[0], text(f32)
    mr.assert_same_bricks(f32.export_bricks(), m["bricks"])
    # NULL stats are fine for the merge itself
    rc, _ = raw_call(dst, src, eye, mode=0, stats=False)
    assert rc == _abi.TSDF_OK, text(dst)
    f32.close()
    dst.close()


def test_an_open_border_reduce_is_refused():
    import torch
    from tsdf_map import _abi
    a, b, src = hip(), hip(), hip()
    for v in (a, b, src):
        v.import_bricks(*bricks_of([[1, 2, 3]], [0.1], [2.0], F(TAU)))
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
    eye = POSES["identity"]
    rc, _ = raw_call(b, src, eye)
    assert rc == _abi.TSDF_EINVAL and text(b) == (
        "merge: a border reduce is open on the destination context: commit or abort it first "
        "(tsdf_border_commit_device)")
    rc, _ = raw_call(src, b, eye)
    assert rc == _abi.TSDF_EINVAL and text(src) == (
        "merge: a border reduce is open on the source context: commit or abort it first "
        "(tsdf_border_commit_device)")
    b.border_commit(False)
    rc, st = raw_call(src, b, eye, mode=0)
    assert rc == _abi.TSDF_OK and st["overlap_voxels"] == 1, text(src)
    for v in (a, b, src):
        v.close()


def test_contexts_on_different_devices_are_refused():
    import torch
    from tsdf_map import _abi
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    a, b = hip(device_id=0), hip(device_id=1)
    rc, _ = raw_call(a, b, POSES["identity"])
    assert rc == _abi.TSDF_EINVAL and text(a) == \
        "merge: the contexts are on different devices (0 and 1)"
    a.close()
    b.close()


# ---- the Python layer ----------------------------------------------------------------------------

def test_transformed_there_and_back(maps):
    m = maps["vdbfusion_f64"]
    T = mr.rigid(t=(3 * float(F(VS)), -5 * float(F(VS)), float(F(VS))))
    there = m["crop"].transformed(T, mode="nearest")
    assert there.semantics == "vdbfusion_f64" and there.voxel_size == VS
    assert there.params.max_bricks == m["crop"].params.max_bricks
    ijk = there.export_voxels()[0]
    assert np.array_equal(ijk, m["voxels"][0] + np.array([3, -5, 1]))
    back = there.transformed(np.vstack([mr.invert(T), [0, 0, 0, 1]]), mode="nearest")
    mr.assert_same_bricks(back.export_bricks(), m["bricks"])
    mr.assert_same_bricks(m["crop"].export_bricks(), m["bricks"])
    with pytest.raises(ValueError):
        m["crop"].transformed(np.eye(3))
    with pytest.raises(ValueError):
        m["crop"].transformed(T, mode="cubic")
    there.close()
    back.close()


def test_fuse_submaps_equals_three_merges(maps):
    from tsdf_map import fuse_submaps
    c, s, w = maps["vdbfusion_f64"]["full"]
    third = len(c) // 3
    subs = []
    for k in range(3):
        v = hip()
        v.import_bricks(*[a[k * third:(k + 1) * third + 40] for a in (c, s, w)])  # overlapping
        subs.append(v)
    # (poses close to each other, so that the shared bricks of neighbouring crops meet again)
    poses = [POSES["identity"], POSES["half_voxel"], mr.rigid((0.0, 0.0, 1.0), (-0.1, 0.05, 0.0))]
    fused, counts = fuse_submaps(subs, poses, mode="nearest", min_weight=0.0)
    ref = hip()
    want = [ref.merge_from(v, T, mode="nearest") for v, T in zip(subs, poses)]
    assert counts == want and counts[1]["overlap_voxels"] > 0 and len(counts) == 3
    mr.assert_same_bricks(fused.export_bricks(), ref.export_bricks())
    assert fused.semantics == subs[0].semantics
    # into an existing volume: the same again on top
    again, more = fuse_submaps(subs[:1], poses[:1], into=ref, mode="nearest")
    assert again is ref and more[0]["new_bricks"] == 0
    with pytest.raises(ValueError):
        fuse_submaps(subs, poses[:2])
    for v in subs + [fused, ref]:
        v.close()
