"""The integrate walks at the edge of the index domain and on far points (include/tsdf_hip.h "Index
domain").

A voxel outside |i| < 2^23 is never written; TSDF_VB_MERGED drops points whose voxel lies outside
|i| < 2^20; a ray whose index-space start (Voxblox: start, end or hit point) is not finite or
reaches 2^30 is dropped whole and not counted.  Every walk kernel decides per wave whether its rays
need the per-voxel domain check; a scan whose origin stands 3 m inside the +x edge and 2 m inside
the -y edge mixes both kinds of lanes in the same waves.

CPU part: the oracle against a per-sample numpy restatement with the domain as a plain mask
(tests/walkref.py), and against metamorphic expectations for far points (the field and the ray
count are those of the ordinary points alone).  GPU part: every front end against the oracle, bit
for bit, and the read side on the edge map.  All assertions are bitwise.
"""
import functools
import math
import time

import numpy as np
import pytest

import oracle
import sampleref as sr
import walkref
from conftest import decimate

VS, TAU = 0.05, 0.15
LIM = 1 << 23      # the index domain
MG_LIM = 1 << 20   # the Merged bundling keys
F = np.float32

SEMANTICS = ["vdbfusion_f64", "vdbfusion", "voxblox"]


def ora(**kw):
    for k in ("max_batch", "pipeline", "walk", "max_points", "max_bricks", "max_bricks_hard"):
        kw.pop(k, None)
    return oracle.OracleTSDFVolume(VS, TAU, **kw)


def hip(**kw):
    from tsdf_map import HipTSDFVolume
    kw.setdefault("max_bricks", 1 << 16)
    kw.setdefault("max_points", 1 << 14)
    return HipTSDFVolume(VS, TAU, **kw)


def same_field(a, b):
    (ai, as_, aw), (bi, bs, bw) = a, b
    assert ai.shape == bi.shape, (ai.shape, bi.shape)
    assert np.array_equal(ai, bi)
    assert np.array_equal(np.asarray(aw, F).view(np.uint32), np.asarray(bw, F).view(np.uint32))
    assert np.array_equal(np.asarray(as_, F).view(np.uint32), np.asarray(bs, F).view(np.uint32))
    return ai.shape[0]


def assert_bitwise(g, o):
    return same_field(g.export_voxels(), o.export_voxels())


# ---- inputs ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sim():
    from tsdf_map.scan_gen import OusterSim
    return OusterSim()


def edge_shift(lim):
    """The shift that puts scan 0's origin 3 m inside the +x edge (L = lim vs) and 2 m inside the
    -y edge."""
    org = _sim().scan(0)[1]
    L = lim * VS
    return np.array([L - 3.0 - org[0], -(L - 2.0) - org[1], 0.0])


@functools.lru_cache(maxsize=None)
def edge_scan(k=0, lim=LIM, dec=16):
    """sim.scan(k) decimated, shifted in float64 and then rounded to fp32; its float64 origin."""
    pts, org = _sim().scan(k)
    sh = edge_shift(lim)
    p = np.ascontiguousarray((decimate(pts, dec).astype(np.float64) + sh).astype(F))
    p.setflags(write=False)
    return p, org + sh


def voxel_of(p):
    return np.floor(np.asarray(p, np.float64) / VS)


def outside(p, lim):
    return np.any(np.abs(voxel_of(p)) >= lim, axis=1)


Q_TILT = np.array([math.sin(0.15), 0.05, 0.1, math.cos(0.15)])  # a pose: 1/z^2 weights differ per ray


def posed(org, j=0):
    q = Q_TILT + np.array([0.0, 0.02 * j, 0.0, 0.0])
    return np.concatenate([org, q])


# The far-point cloud: ~200 ordinary points mixed with far and non-finite ones.  BIG0 is 2^30 vs
# pushed up by 2^-20 (relative), so that a band start 3 voxels before the point still rounds to
# >= 2^30 in fp32 (ulp 128 there) in every semantics: the first magnitude the rule drops for sure.
BIG0 = 2.0 ** 30 * VS * (1.0 + 2.0 ** -20)
FAR_MAGS = (BIG0, 2e8, 1e20, 1e30, 3e38)


def far_points():
    out = []
    for m in FAR_MAGS:
        for a in range(3):
            for s in (1.0, -1.0):
                p = [1.5, -2.5, 0.5]
                p[a] = s * m
                out.append(p)
        out += [[m, m, m], [-m, m, 1.0], [2.0, -m, -m], [m, -3.0, m]]
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            p = [1.5, -2.5, 0.5]
            p[a] = bad
            out.append(p)
    out += [[np.nan] * 3, [np.inf, -np.inf, np.nan], [np.inf, 1e30, -3e38]]
    return np.array(out, np.float64).astype(F)


@functools.lru_cache(maxsize=None)
def far_cloud():
    """(mixed cloud, ordinary points alone, origin): the far points are spread through the ordinary
    ones, so that a wave holds both."""
    pts, org = _sim().scan(0)
    ordinary = decimate(pts, 655)
    far = far_points()
    assert 190 <= ordinary.shape[0] <= 210 and far.shape[0] > 50
    mixed = np.empty((ordinary.shape[0] + far.shape[0], 3), F)
    slots = np.linspace(0, mixed.shape[0] - 1, far.shape[0]).astype(np.int64)
    is_far = np.zeros(mixed.shape[0], bool)
    is_far[slots] = True
    mixed[is_far] = far
    mixed[~is_far] = ordinary
    return mixed, ordinary, org


def sem_kw(name):
    """The four semantics of the walk kernels (internal 2, 0, 1, 3) and whether scans carry a pose."""
    if name == "voxblox":
        return dict(semantics="voxblox", use_const_weight=True), False
    if name == "voxblox_z2":
        return dict(semantics="voxblox", use_const_weight=False), True
    return dict(semantics=name), False


def edge_scans(n, pose, lim=LIM, dec=16):
    out = []
    for k in range(n):
        p, org = edge_scan(k, lim, dec)
        out.append((p, posed(org, k) if pose else org))
    return out


@functools.lru_cache(maxsize=None)
def edge_ref(name, n, **extra):
    """The oracle's edge map of the first n edge scans: (volume, exported field, stats)."""
    kw, pose = sem_kw(name)
    o = ora(**kw, **dict(extra))
    for p, e in edge_scans(n, pose):
        o.integrate(p, e)
    return o, o.export_voxels(), o.stats()


# ---- 1. CPU: the oracle at the edge -------------------------------------------------------------------

def check_edge_field(ijk, p, lim):
    """The conditions that keep every comparison on the edge scan from being vacuous."""
    out = outside(p, lim)
    assert out.mean() >= 0.25 and (~out).mean() >= 0.25, out.mean()
    assert np.abs(ijk).max() == lim - 1 and np.all(np.abs(ijk) < lim)
    on_x = int((ijk[:, 0] == lim - 1).sum())
    on_y = int((ijk[:, 1] == -(lim - 1)).sum())
    assert on_x > 0 and on_y > 0, (on_x, on_y)
    return int(out.sum()), on_x, on_y


@pytest.mark.parametrize("semantics", SEMANTICS)
def test_oracle_edge_scan_is_the_clipped_restatement(semantics):
    """The oracle's field of the edge scan equals, bit for bit, the per-sample numpy restatement
    with the samples outside |i| < 2^23 masked away; both extreme planes are populated."""
    p, org = edge_scan()
    kw, _ = sem_kw(semantics)
    o = ora(**kw)
    o.integrate(p, org)
    got = o.export_voxels()
    n_out, on_x, on_y = check_edge_field(got[0], p, LIM)
    ref = walkref.integrate_one_scan(p, org, semantics, VS, TAU, lim=LIM)
    free = walkref.integrate_one_scan(p, org, semantics, VS, TAU, lim=None)
    print("%s: %d of %d points outside, %d voxels kept of %d unclipped, %d on +x, %d on -y" % (
        semantics, n_out, p.shape[0], got[0].shape[0], free[0].shape[0], on_x, on_y))
    assert free[0].shape[0] > 2 * ref[0].shape[0] > 20000  # the clip is what the test is about
    assert same_field(got, ref) > 10000
    assert o.stats()["n_rays_total"] == p.shape[0]  # |start| < 2^30: clipped voxel by voxel, counted
    assert o.num_bricks() == np.unique(got[0] >> 3, axis=0).shape[0]


@pytest.mark.parametrize("kw", [dict(use_const_weight=True), dict(use_const_weight=False)],
                         ids=["const", "z2"])
def test_oracle_merged_drops_points_beyond_2_20(kw):
    """TSDF_VB_MERGED at its own edge (bundling keys hold |i| < 2^20): the points whose voxel lies
    beyond are dropped before bundling, so the field is that of the points inside alone, and the
    bundles' walks still reach the last voxels."""
    p, org = edge_scan(0, MG_LIM)
    e = posed(org) if not kw["use_const_weight"] else org
    o = ora(semantics="voxblox", method="merged", **kw)
    o.integrate(p, e)
    got = o.export_voxels()
    # the bundling key of a point is floor(p / vs + 1e-6) in fp32
    key = np.floor(p * (F(1.0) / F(VS)) + F(1e-6))
    inside = np.all(np.abs(key) < MG_LIM, axis=1)
    assert inside.mean() >= 0.25 and (~inside).mean() >= 0.25
    kept = ora(semantics="voxblox", method="merged", **kw)
    kept.integrate(np.ascontiguousarray(p[inside]), e)
    assert same_field(got, kept.export_voxels()) > 10000
    assert o.stats()["n_rays_total"] == kept.stats()["n_rays_total"] > 1000
    ijk = got[0]
    # a bundle's ray ends tau behind its mean point: voxels up to tau / vs + 1 past the last key
    assert MG_LIM - 1 <= np.abs(ijk).max() <= MG_LIM + 4
    assert (ijk[:, 0] >= MG_LIM - 1).any() and (ijk[:, 1] <= -(MG_LIM - 1)).any()


@pytest.mark.parametrize("semantics", SEMANTICS)
@pytest.mark.parametrize("where", ["past_the_edge", "utm"])
def test_oracle_scan_wholly_outside_is_an_empty_map(semantics, where):
    pts, org = _sim().scan(0)
    kw, _ = sem_kw(semantics)
    sh = np.array([LIM * VS + 5.0 - org[0], 0.0, 0.0]) if where == "past_the_edge" else \
        np.array([3.5e5, 4.0e6, 0.0])
    p = (decimate(pts, 16).astype(np.float64) + sh).astype(F)
    if where == "past_the_edge":  # the rays that look back into the domain are not this case
        p = np.ascontiguousarray(p[voxel_of(p)[:, 0] >= LIM + 4])
        assert p.shape[0] > 2000
    o = ora(**kw)
    o.integrate(p, org + sh)  # TSDF_OK, or the wrapper raises
    assert o.num_bricks() == 0 and o.export_voxels()[0].shape[0] == 0
    if where == "utm":  # 8 10^7 voxels out: inside the far-ray rule, so walked, clipped and counted
        assert o.stats()["n_rays_total"] == p.shape[0]


@pytest.mark.parametrize("max_range", [math.inf, 30.0])
@pytest.mark.parametrize("semantics", SEMANTICS + ["voxblox_z2", "merged"])
def test_oracle_far_points_leave_the_field_alone(semantics, max_range):
    """Metamorphic: far (>= 2^30 voxels on an axis) and non-finite points are dropped like
    range-filtered ones, so the field and the ray count are those of the ordinary points alone.
    With max_range 30 Voxblox turns points beyond it into clearing rays: a far point makes none."""
    mixed, ordinary, org = far_cloud()
    if semantics == "merged":
        kw, pose = dict(semantics="voxblox", method="merged"), True
    else:
        kw, pose = sem_kw(semantics)
    e = posed(org) if pose else org
    a, b = ora(max_range=max_range, **kw), ora(max_range=max_range, **kw)
    a.integrate(mixed, e)
    b.integrate(ordinary, e)
    assert same_field(a.export_voxels(), b.export_voxels()) > 500
    assert a.stats()["n_rays_total"] == b.stats()["n_rays_total"] > 100
    if max_range == math.inf and semantics != "merged":
        assert b.stats()["n_rays_total"] == ordinary.shape[0]


@pytest.mark.parametrize("semantics", SEMANTICS)
def test_oracle_far_points_inside_the_rule_are_walked(semantics):
    """The rule's other side: a point 2^29 voxels out is an ordinary ray.  Its voxels all lie
    outside the domain, so it writes nothing, but it is counted."""
    _, ordinary, org = far_cloud()
    m = 2.0 ** 29 * VS
    far = np.array([[m, 1, 1], [-m, 1, 1], [1, m, 1], [1, -m, 1], [1, 1, m], [1, 1, -m]], F)
    kw, _ = sem_kw(semantics)
    a, b = ora(**kw), ora(**kw)
    a.integrate(np.concatenate([far[:3], ordinary, far[3:]]), org)
    b.integrate(ordinary, org)
    assert same_field(a.export_voxels(), b.export_voxels()) > 500
    assert a.stats()["n_rays_total"] == ordinary.shape[0] + 6


@pytest.mark.parametrize("semantics", SEMANTICS)
def test_oracle_carving_walk_ends_after_max_dda_steps(semantics):
    """KAT of MAX_DDA_STEPS = 2^20: with carving and max_range = inf a ray to a point 10^5 m away
    (2 10^6 voxels, inside the far-ray rule) is walked for exactly 2^20 voxels from the origin."""
    kw, _ = sem_kw(semantics)
    o = ora(space_carving=True, **kw)
    t = time.perf_counter()
    o.integrate(np.array([[1e5, 0.0125, 0.0125]], F), np.array([0.0125, 0.0125, 0.0125]))
    ijk, s, w = o.export_voxels()
    print("%s: %d voxels carved in %.2f s" % (semantics, ijk.shape[0], time.perf_counter() - t))
    assert o.stats()["n_rays_total"] == 1
    assert ijk.shape[0] == 1 << 20
    assert np.array_equal(ijk[:, 0], np.arange(1 << 20)) and not ijk[:, 1:].any()
    assert np.all(s == F(TAU)) and np.all(w == 1)


# ---- 2. GPU: the kernels against the oracle -------------------------------------------------------------

GPU_SEMANTICS = ["vdbfusion_f64", "vdbfusion", "voxblox", "voxblox_z2"]


def check_gpu(g, ref, what):
    o, field, st = ref
    g.sync()
    assert same_field(g.export_voxels(), field) > 10000, what
    gs = g.stats()
    assert gs["n_rays_total"] == st["n_rays_total"], what
    assert g.num_bricks() == o.num_bricks(), what


@pytest.mark.gpu
@pytest.mark.parametrize("semantics", GPU_SEMANTICS)
def test_gpu_edge_scan_two_walk(semantics):
    """k_count / k_place one scan per batch: the checked and the unchecked walk in the same waves."""
    kw, pose = sem_kw(semantics)
    ref = edge_ref(semantics, 1)
    check_edge_field(ref[1][0], edge_scan()[0], LIM)
    g = hip(max_batch=1, **kw)
    for p, e in edge_scans(1, pose):
        g.integrate(p, e)
    check_gpu(g, ref, "two-walk")


@pytest.mark.gpu
@pytest.mark.parametrize("semantics", GPU_SEMANTICS)
def test_gpu_edge_scans_device_batch_of_12(semantics):
    """A 12-scan device batch (more than 8 scans: k_integrate, not k_integrate_small, fuses)."""
    import torch
    kw, pose = sem_kw(semantics)
    ref = edge_ref(semantics, 12)
    scans = edge_scans(12, pose)
    offs = np.cumsum([0] + [p.shape[0] for p, _ in scans]).astype(np.uint64)
    d = torch.from_numpy(np.concatenate([p for p, _ in scans])).to("cuda:0")
    torch.cuda.synchronize()
    g = hip(max_batch=12, max_points=1 << 17, **kw)
    g.integrate_batch_device(d.data_ptr(), offs, np.stack([e for _, e in scans]))
    check_gpu(g, ref, "device batch")
    assert g.stats()["n_batches"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("semantics", GPU_SEMANTICS)
def test_gpu_edge_scans_small_batch_and_wide_count(semantics, monkeypatch):
    """3 scans per batch through k_integrate_small with the 1024-lane k_count, and with both
    toggled off (TSDF_SMALL_NS=0, TSDF_COUNT_WIDE=0), as test_small_batch_kernel_bitwise sets them."""
    kw, pose = sem_kw(semantics)
    ref = edge_ref(semantics, 3)
    for small in ("8", "0"):
        monkeypatch.setenv("TSDF_SMALL_NS", small)
        monkeypatch.setenv("TSDF_COUNT_WIDE", "256" if small != "0" else "0")
        g = hip(max_batch=3, **kw)
        for p, e in edge_scans(3, pose):
            g.integrate(p, e)
        check_gpu(g, ref, small)


@pytest.mark.gpu
@pytest.mark.parametrize("semantics", ["vdbfusion_f64", "vdbfusion", "voxblox"])
def test_gpu_edge_scans_single_walk(semantics):
    """walk="single" where the band allows it (no per-sample weights): k_walk's own dispatch."""
    kw, pose = sem_kw(semantics)
    ref = edge_ref(semantics, 3)
    g = hip(max_batch=3, walk="single", **kw)
    g.set_profiling(True)
    for p, e in edge_scans(3, pose):
        g.integrate(p, e)
    check_gpu(g, ref, "single")
    launches = g.stats()["kernel_launches"]
    assert launches["walk"] > 0 and launches["count"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("semantics", GPU_SEMANTICS)
def test_gpu_edge_scans_pipeline_2(semantics):
    kw, pose = sem_kw(semantics)
    ref = edge_ref(semantics, 12)
    g = hip(max_batch=3, pipeline=2, **kw)
    for p, e in edge_scans(12, pose):
        g.integrate(p, e)
    check_gpu(g, ref, "pipeline=2")


@pytest.mark.gpu
@pytest.mark.parametrize("semantics", GPU_SEMANTICS)
def test_gpu_edge_scan_carving(semantics):
    """Carving (more than 4 pairs per ray: the walks that always check) across both edges."""
    kw, pose = sem_kw(semantics)
    p, org = edge_scan(0, LIM, 64)
    e = posed(org) if pose else org
    extra = dict(space_carving=True, max_range=30.0)
    o = ora(**kw, **extra)
    o.integrate(p, e)
    ijk = o.export_voxels()[0]
    assert np.abs(ijk).max() == LIM - 1 and (ijk[:, 0] == LIM - 1).any() and \
        (ijk[:, 1] == -(LIM - 1)).any()
    g = hip(max_batch=1, max_bricks=1 << 17, **kw, **extra)
    g.integrate(p, e)
    g.sync()
    assert assert_bitwise(g, o) > 50000
    assert g.stats()["n_rays_total"] == o.stats()["n_rays_total"]
    assert g.num_bricks() == o.num_bricks()


@pytest.mark.gpu
@pytest.mark.parametrize("const", [True, False], ids=["const", "z2"])
def test_gpu_merged_at_its_edge(const):
    kw = dict(semantics="voxblox", method="merged", use_const_weight=const)
    o, g = ora(**kw), hip(max_batch=3, **kw)
    for k in range(3):
        p, org = edge_scan(k, MG_LIM)
        e = org if const else posed(org, k)
        o.integrate(p, e)
        g.integrate(p, e)
    g.sync()
    ijk = o.export_voxels()[0]
    assert (ijk[:, 0] >= MG_LIM - 1).any() and (ijk[:, 1] <= -(MG_LIM - 1)).any()
    assert np.abs(ijk).max() <= MG_LIM + 4
    assert assert_bitwise(g, o) > 10000
    assert g.stats()["n_rays_total"] == o.stats()["n_rays_total"]
    assert g.num_bricks() == o.num_bricks()


@pytest.mark.gpu
@pytest.mark.parametrize("max_range", [math.inf, 30.0])
@pytest.mark.parametrize("semantics", GPU_SEMANTICS)
def test_gpu_far_points_and_a_scan_wholly_outside(semantics, max_range):
    """One 3-scan batch: an ordinary scan, the far-point cloud, a scan wholly outside the domain.
    The pool is fixed at 4x the oracle's brick count, so a walk that invents bricks reports
    TSDF_ENOMEM instead of growing.  Equal to the oracle and to the batch without the far points."""
    kw, pose = sem_kw(semantics)
    mixed, ordinary, org = far_cloud()
    p0, o0 = _sim().scan(1)
    p0 = decimate(p0, 64)
    sh = np.array([LIM * VS + 5.0 - org[0], 0.0, 0.0])
    gone = (decimate(_sim().scan(2)[0], 64).astype(np.float64) + sh).astype(F)
    gone = np.ascontiguousarray(gone[voxel_of(gone)[:, 0] >= LIM + 4])  # no ray back into the domain
    assert gone.shape[0] > 500

    def ext(x, j):
        return posed(x, j) if pose else x

    if max_range == math.inf:  # the rule's other side: 2^29 voxels out, walked and clipped
        m = 2.0 ** 29 * VS
        mixed = np.concatenate([mixed, np.array([[m, 1, 1], [1, -m, 1], [1, 1, m], [-m, m, -m]], F)])
    with_far = [(p0, ext(o0, 0)), (mixed, ext(org, 1)), (gone, ext(org + sh, 2))]
    without = [(p0, ext(o0, 0)), (ordinary, ext(org, 1))]
    nb, fields = None, []
    for scans in (with_far, without):
        o = ora(max_range=max_range, **kw)
        for p, e in scans:
            o.integrate(p, e)
        nb = nb or o.num_bricks()
        g = hip(max_batch=3, max_bricks=4 * nb, max_bricks_hard=4 * nb, max_range=max_range, **kw)
        for p, e in scans:
            g.integrate(p, e)
        g.sync()  # raises on TSDF_ENOMEM
        assert g.num_bricks() == o.num_bricks() == nb
        assert g.stats()["n_rays_total"] == o.stats()["n_rays_total"]
        fields.append(g.export_voxels())
        assert same_field(fields[-1], o.export_voxels()) > 2000
    same_field(fields[0], fields[1])


# ---- the read side on the edge map -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge_map():
    """The 12 edge scans' map (one decimated scan leaves too few fully observed cubes to mesh or to
    interpolate in): (GPU volume, oracle volume, the oracle's field)."""
    o, field, _ = edge_ref("vdbfusion_f64", 12)
    g = hip(semantics="vdbfusion_f64", max_batch=4)
    for p, e in edge_scans(12, False):
        g.integrate(p, e)
    g.sync()
    yield g, o, field
    g.close()


def corner_box(org):
    """A 64 x 48 x 24 voxel box over the domain's (+x, -y) corner at the sensor's height: it crosses
    both edges."""
    z = int(math.floor(org[2] / VS))
    lo = np.array([LIM - 56, -LIM - 8, z - 12], np.int64)
    return lo, lo + np.array([64, 48, 24])


def carved_corner():
    """The oracle's carved edge map (the free space the rays cross fills the corner) and its dense
    read-out of the corner box, checked: observed voxels inside, background outside the domain."""
    p, org = edge_scan(0, LIM, 64)
    o = ora(semantics="vdbfusion_f64", space_carving=True, max_range=30.0)
    o.integrate(p, org)
    lo, hi = corner_box(org)
    os_, ow = o.query_dense(lo, hi)
    x, y = np.arange(lo[0], hi[0]), np.arange(lo[1], hi[1])
    assert np.count_nonzero(ow) > 1000
    assert ow[:, :, x == LIM - 1].any() and ow[:, y == -(LIM - 1), :].any()
    assert not ow[:, :, x >= LIM].any() and not ow[:, y <= -LIM, :].any()
    assert np.all(os_[:, :, x >= LIM] == F(TAU)) and np.all(os_[:, y <= -LIM, :] == F(TAU))
    return (p, org), (lo, hi), (os_, ow)


def test_oracle_query_dense_across_both_edges():
    carved_corner()


@pytest.mark.gpu
def test_gpu_query_dense_across_both_edges():
    (p, org), (lo, hi), (os_, ow) = carved_corner()
    g = hip(semantics="vdbfusion_f64", space_carving=True, max_range=30.0, max_bricks=1 << 17)
    g.integrate(p, org)
    gs, gw = g.query_dense(lo, hi)
    assert np.array_equal(gw, ow)
    assert np.array_equal(gs.view(np.uint32), os_.view(np.uint32))


@pytest.mark.gpu
def test_gpu_brick_roundtrip_at_the_extreme_coordinates(edge_map):
    g, o, _ = edge_map
    coords, s, w = g.export_bricks()
    assert coords[:, 0].max() == (1 << 20) - 1 and coords[:, 1].min() == -(1 << 20)
    for x, y in zip((coords, s, w), o.export_bricks()):
        assert np.array_equal(x, y)
    b = hip(semantics="vdbfusion_f64")
    b.import_bricks(coords, s, w)
    for x, y in zip(b.export_bricks(), (coords, s, w)):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))


@pytest.mark.gpu
def test_gpu_mesh_at_the_edge(edge_map):
    """The last brick has no +x neighbour: its outer cubes are not meshed, as in the oracle's soup."""
    g, o, _ = edge_map
    vo, _ = o.extract_triangle_mesh()
    vg, _ = g.extract_triangle_mesh()
    assert vo.shape[0] > 10000
    # triangles inside the last bricks before +x and -y
    assert (vo[:, 0] > (LIM - 8) * VS).sum() > 100 and (vo[:, 1] < -(LIM - 8) * VS).sum() > 100
    assert vg.shape == vo.shape and np.array_equal(vg.view(np.uint32), vo.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_gpu_sample_on_the_edge_maps_voxel_centres(edge_map, mode):
    g, _, field = edge_map
    ref_field = sr.Field(field, VS, F(TAU))
    ijk = field[0].astype(np.float64)
    p = np.ascontiguousarray(((ijk + 0.5) * VS).astype(F))
    ref = sr.sample(ref_field, p, sr.NEAREST if mode == "nearest" else sr.TRILINEAR)
    v = ref[3].astype(bool)
    assert v.sum() > 1000 and (~v).sum() > 100, (v.sum(), (~v).sum())
    gs, gw, gg, gv = g.sample(p, mode=mode)
    assert np.array_equal(np.asarray(gv).astype(np.uint8), ref[3])
    for a, b in zip((gs, gw, gg), ref[:3]):
        assert np.array_equal(np.ascontiguousarray(a, F).view(np.uint32),
                              np.ascontiguousarray(b, F).view(np.uint32))
