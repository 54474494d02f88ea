"""The distance field on the GPU (include/tsdf_hip_esdf.h) against tests/esdfref.py, bit for bit:
dist as uint32, flags as uint8.  The reference reads the GPU volume's own query_dense, so what
test_esdf_ref.py pins on the CPU is what the kernels are held to here.  No box has more than about
3 * 10^5 voxels, but the three of tests/pastcap.py, which take each kernel past its grid cap."""
import ctypes as C

import numpy as np
import pytest

import esdfref as er
import pastcap as pc
import sampleref as sr

pytestmark = pytest.mark.gpu

F = np.float32
VS = sr.VOXEL_SIZE
TAU = sr.SDF_TRUNC
SMALL = dict(max_bricks=1 << 12, max_points=1 << 12, max_batch=4)


def i64(a):
    return np.ascontiguousarray(np.asarray(a, np.int64).reshape(3))


def text(v):
    return v._lib.tsdf_last_error(v._ctx).decode()


def max_dist(radius):
    """A max_dist whose ceil(max_dist / VS) is `radius`."""
    return (radius - 0.5) * VS


def host_call(v, lo, hi, radius, band, mw, with_flags=True):
    """tsdf_esdf_dense through ctypes: (rc, dist, flags or None), [z, y, x]."""
    from tsdf_map import _abi
    lo, hi = i64(lo), i64(hi)
    n = np.maximum(hi - lo, 0)
    dist = np.full((n[2], n[1], n[0]), np.nan, F)
    flags = np.full(dist.shape, 0xEE, np.uint8) if with_flags else None
    rc = v._lib.tsdf_esdf_dense(v._ctx, lo.ctypes.data_as(_abi.L3), hi.ctypes.data_as(_abi.L3),
                                radius, band, mw, dist.ctypes.data_as(_abi.FP),
                                flags.ctypes.data_as(_abi.U8P) if with_flags else None)
    return rc, dist, flags


def check_box(v, lo, hi, radius, band=VS, mw=0.0, ref=None):
    """Both entry points, with and without flags, against the reference; returns the reference."""
    from tsdf_map import _abi
    if ref is None:
        ref = er.of_volume(v, lo, hi, radius, band, mw)
    md = max_dist(radius)
    er.assert_same(v.esdf(lo, hi, md, site_band=band, min_weight=mw), ref)
    d, f = v.esdf_device(lo, hi, md, site_band=band, min_weight=mw)
    er.assert_same((d.cpu().numpy(), f.cpu().numpy()), ref)
    d, f = v.esdf_device(lo, hi, md, site_band=band, min_weight=mw, flags=False)
    assert f is None
    er.assert_same((d.cpu().numpy(), None), ref)
    rc, d, f = host_call(v, lo, hi, radius, band, mw, with_flags=False)
    assert rc == _abi.TSDF_OK, text(v)
    er.assert_same((d, None), ref)
    return ref


@pytest.fixture(scope="module")
def maps(scan0):
    from tsdf_map import HipTSDFVolume
    pts, org = scan0
    out = {}
    for sem, p in (("vdbfusion_f64", pts), ("voxblox", np.ascontiguousarray(pts[::2]))):
        v = HipTSDFVolume(VS, TAU, semantics=sem)
        v.integrate(p, org)
        v.sync()
        out[sem] = v
    yield out
    for v in out.values():
        v.close()


@pytest.fixture(scope="module")
def centre(scan0):
    c = er.fixture_centre(scan0)
    assert tuple(c) == (80, -51, -18)
    return c


@pytest.fixture(scope="module")
def fields(maps, centre):
    """(S, W) of the fixture box per map, read once."""
    lo, hi = er.fixture_box(centre)
    return {sem: v.query_dense(lo, hi) for sem, v in maps.items()}


@pytest.mark.parametrize("band", [VS, VS / 2])
@pytest.mark.parametrize("min_weight", [0.0, 2.0])
@pytest.mark.parametrize("radius", [1, 12, 40])
@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_fixture_box_bitwise(maps, fields, centre, sem, radius, min_weight, band):
    lo, hi = er.fixture_box(centre)
    S, W = fields[sem]
    assert S.shape == (33, 80, 97)
    ref = er.esdf(S, W, VS, radius, band, min_weight)
    n_site, n_cap = ((ref[1] & er.SITE) != 0).sum(), ((ref[1] & er.CAPPED) != 0).sum()
    print("%s R %d min_weight %g band %g: %d sites, %d capped, %d negative"
          % (sem, radius, min_weight, band, n_site, n_cap, np.signbit(ref[0]).sum()))
    assert n_site >= 100 and np.signbit(ref[0]).sum() >= 100
    if radius < 40:
        # (capped voxels, and uncapped ones that are no sites: at R = 1 a site's 6 neighbours)
        assert n_cap >= 10000 and (ref[1] & er.CAPPED == 0).sum() >= 2 * n_site
    elif min_weight == 0.0 and band == VS:
        assert n_cap == 0  # at R = 40 every voxel of the box has a site in reach
    check_box(maps[sem], lo, hi, radius, band, min_weight, ref=ref)


SHAPES = [
    ((1, 1, 1), 3), ((97, 1, 1), 12), ((1, 80, 33), 12), ((2, 3, 130), 12),
    ((67, 45, 21), 12),       # no extent a multiple of 8 or 64
    ((600, 9, 5), 20),        # a line longer than any one workgroup's tile
    ((67, 45, 21), 128),      # every extent below R
    ((67, 45, 21), 1),
    ((2, 3, 130), 48), ((2, 3, 130), 49),   # either side of the segment-length threshold
    ((130, 70, 3), 64),       # 64-voxel segments along y, more than one of them
]


@pytest.mark.parametrize("shape,radius", SHAPES)
def test_tiling_shapes(maps, centre, shape, radius):
    v = maps["vdbfusion_f64"]
    n = np.array(shape)
    lo = centre - n // 2
    ref = check_box(v, lo, lo + n, radius)
    if n.prod() > 1000:
        assert ((ref[1] & er.SITE) != 0).sum() >= 10
    assert ref[0].shape == shape[::-1]


def synthetic(voxels, sem="vdbfusion_f64"):
    from tsdf_map import HipTSDFVolume
    v = HipTSDFVolume(VS, TAU, semantics=sem, **SMALL)
    if voxels:
        v.import_bricks(*er.make_bricks(voxels, 0.0 if sem == "voxblox" else F(TAU)))
    return v


@pytest.mark.parametrize("name", list(pc.ESDF_BOXES))
def test_past_the_grid_cap(name):
    """Thin boxes with more tiles than ESDF_GRID_CAP in one or two passes: the voxels of the later
    trips hold seeded sites and uncapped voxels, on either side of the trip's boundary."""
    voxels, lo, hi, radius, (S, W), ref = pc.esdf_case(name)
    sides = pc.esdf_sides(name)
    print("%s %s R %d: %s" % (name, tuple((hi - lo).tolist()), radius,
                              {k: d["tiles"] for k, d in sides.items()}))
    for kernel in pc.ESDF_BOXES[name]["past"]:
        print("  %s: %s" % (kernel, sides[kernel]))
    pc.assert_esdf_past_cap(name, sides)
    v = synthetic(voxels)
    gs, gw = v.query_dense(lo, hi)  # the volume holds the field the reference was computed on
    assert np.array_equal(er.bits(gs), er.bits(S)) and np.array_equal(er.bits(gw), er.bits(W))
    check_box(v, lo, hi, radius, ref=ref)
    v.close()


def test_single_site_in_a_brick_corner():
    """The site is local voxel (7, 7, 7) of a brick; the box spans its 7 neighbour bricks."""
    v = synthetic({(7, 7, 7): (-0.01, 1.0)})
    for radius in (5, 12):
        ref = check_box(v, [0, 0, 0], [16, 16, 16], radius)
        assert er.bits(ref[0])[7, 7, 7] == 0x80000000 and ref[1][7, 7, 7] == 3
        assert ref[0][8, 8, 8] == np.sqrt(F(3)) * F(VS) and ref[1][8, 8, 8] == 0
        assert (ref[1][0, 7, 7] == er.CAPPED) == (radius == 5)  # 7 voxels below the site
    v.close()


def test_sites_on_corners_and_faces():
    lo, hi = np.array([-5, 3, -9]), np.array([14, 16, 2])
    last = hi - 1
    vox = {}
    for x in (lo[0], last[0]):
        for y in (lo[1], last[1]):
            for z in (lo[2], last[2]):
                vox[(int(x), int(y), int(z))] = (0.02, 1.0)
    mid = (lo + last) // 2
    for a in range(3):
        for e in (lo[a], last[a]):
            p = mid.copy()
            p[a] = e
            vox[tuple(int(q) for q in p)] = (-0.02, 1.0)
    v = synthetic(vox)
    for radius in (3, 9, 20):
        ref = check_box(v, lo, hi, radius)
        assert ((ref[1] & er.SITE) != 0).sum() == 14
    v.close()


def test_empty_map_reads_capped():
    v = synthetic({})
    for radius in (1, 7, 128):
        ref = check_box(v, [-3, -4, -5], [9, 3, 2], radius)
        assert (ref[1] == er.CAPPED).all()
        assert (er.bits(ref[0]) == er.bits(np.sqrt(F(radius * radius)) * F(VS))).all()
    v.close()


def test_index_domain_edge():
    """Voxels at |i| >= 2^23 read unobserved; the last voxel inside the domain may be a site."""
    lim = 1 << 23
    v = synthetic({(lim - 1, 2, -3): (0.0, 1.0), (-lim + 1, 0, 0): (0.01, 1.0)})
    ref = check_box(v, [lim - 6, -2, -6], [lim + 7, 5, 0], 9)  # straddles +2^23 on x
    assert ref[1][3, 4, 5] == 3 and (ref[1][:, :, 6:] & er.OBSERVED == 0).all()
    assert ref[0][3, 4, 12] == F(7) * F(VS)
    ref = check_box(v, [-lim - 4, -2, -2], [-lim + 3, 3, 3], 4)  # straddles -2^23
    assert ((ref[1] & er.SITE) != 0).sum() == 1
    for lo, hi in (([lim, 0, 0], [lim + 9, 4, 3]), ([0, -lim - 9, 0], [3, -lim, 5]),
                   ([1 << 40, -(1 << 50), 0], [(1 << 40) + 5, -(1 << 50) + 6, 7])):
        ref = check_box(v, lo, hi, 4)  # wholly outside
        assert (ref[1] == er.CAPPED).all() and (ref[0] == F(4) * F(VS)).all()
    v.close()


def test_the_box_is_the_world():
    inner, outer = {(2, 2, 2): (0.01, 1.0)}, {(8, 3, 3): (0.01, 1.0)}
    a, b = synthetic({**inner, **outer}), synthetic(inner)
    lo, hi = [0, 0, 0], [8, 8, 8]
    ra = check_box(a, lo, hi, 10)
    rb = check_box(b, lo, hi, 10)
    er.assert_same(ra, rb)  # a site one voxel outside the box changes nothing in the box
    d, f = a.esdf(lo, [9, 8, 8], max_dist(10))
    assert d[3, 3, 7] == F(VS) and ra[0][3, 3, 7] == np.sqrt(F(25 + 1 + 1)) * F(VS)
    er.assert_same((d, f), er.of_volume(a, lo, [9, 8, 8], 10))
    a.close()
    b.close()


def test_two_calls_give_the_same_bits_and_leave_the_map(maps, centre):
    v = maps["voxblox"]
    lo, hi = er.fixture_box(centre)
    before = v.export_voxels()
    a = v.esdf(lo, hi, max_dist(12))
    b = v.esdf(lo, hi, max_dist(12))
    er.assert_same(a, b)
    d, f = v.esdf_device(lo, hi, max_dist(12))
    er.assert_same((d.cpu().numpy(), f.cpu().numpy()), a)
    after = v.export_voxels()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(er.bits(before[1]), er.bits(after[1]))


@pytest.mark.parametrize("pipeline", [0, 2])
def test_integration_after_a_call_is_still_the_oracles(sim, scan0, centre, pipeline):
    import oracle
    from tsdf_map import HipTSDFVolume
    scans = [(np.ascontiguousarray(p[::8]), o) for p, o in (scan0, sim.scan(1))]
    g = HipTSDFVolume(VS, TAU, pipeline=pipeline)
    o = oracle.OracleTSDFVolume(VS, TAU)
    g.integrate(*scans[0])
    o.integrate(*scans[0])
    lo, hi = er.fixture_box(centre)
    check_box(g, lo, hi, 12)  # (flushes the pending batch itself)
    g.integrate(*scans[1])
    o.integrate(*scans[1])
    gv, ov = g.export_voxels(), o.export_voxels()
    assert np.array_equal(gv[0], ov[0])
    assert np.array_equal(er.bits(gv[1]), er.bits(ov[1]))
    assert np.array_equal(er.bits(gv[2]), er.bits(ov[2]))
    g.close()
    o.close()


def test_refusals(maps):
    import torch
    from tsdf_map import HipTSDFVolume, _abi
    v = maps["vdbfusion_f64"]
    nan, inf = float("nan"), float("inf")
    box = ([0, 0, 0], [4, 3, 2])
    bad = [
        (*box, 0, VS, 0.0), (*box, 129, VS, 0.0), (*box, (1 << 32) - 1, VS, 0.0),
        (*box, 3, -1.0, 0.0), (*box, 3, nan, 0.0), (*box, 3, inf, 0.0),
        (*box, 3, VS, -1.0), (*box, 3, VS, nan),
        ([0, 0, 0], [4, -1, 2], 3, VS, 0.0),
        ([0, 0, 0], [4, 1 << 31, 2], 3, VS, 0.0),
        ([-(1 << 62), 0, 0], [1 << 62, 1, 1], 3, VS, 0.0),
        ([0, 0, 0], [1 << 14, 1 << 14, 2], 3, VS, 0.0),
    ]
    dd = torch.full((24,), 7.0, dtype=torch.float32, device=v.tensor_device)
    df = torch.full((24,), 9, dtype=torch.uint8, device=v.tensor_device)
    for lo, hi, radius, band, mw in bad:
        a, b = i64(lo), i64(hi)
        d, f = np.full(24, 7.0, F), np.full(24, 9, np.uint8)
        rc = v._lib.tsdf_esdf_dense(v._ctx, a.ctypes.data_as(_abi.L3), b.ctypes.data_as(_abi.L3),
                                    radius, band, mw, d.ctypes.data_as(_abi.FP),
                                    f.ctypes.data_as(_abi.U8P))
        assert rc == _abi.TSDF_EINVAL and text(v).startswith("esdf: "), (lo, hi, radius, band, mw)
        assert (d == 7.0).all() and (f == 9).all()
        rc = v._lib.tsdf_esdf_dense_device(v._ctx, a.ctypes.data_as(_abi.L3),
                                           b.ctypes.data_as(_abi.L3), radius, band, mw,
                                           C.c_void_p(dd.data_ptr()), C.c_void_p(df.data_ptr()))
        assert rc == _abi.TSDF_EINVAL and text(v).startswith("esdf: "), (lo, hi, radius, band, mw)
    assert text(v) == "esdf: box above 2^28 voxels"
    # NULL arguments: the bounds, and dist for a box that is not empty
    a, b = i64(box[0]), i64(box[1])
    pa, pb = a.ctypes.data_as(_abi.L3), b.ctypes.data_as(_abi.L3)
    assert v._lib.tsdf_esdf_dense(v._ctx, None, pb, 3, VS, 0.0, None, None) == _abi.TSDF_EINVAL
    assert v._lib.tsdf_esdf_dense(v._ctx, pa, pb, 3, VS, 0.0, None, None) == _abi.TSDF_EINVAL
    assert text(v) == "esdf: null buffer"
    assert v._lib.tsdf_esdf_dense_device(v._ctx, pa, pb, 3, VS, 0.0, None,
                                         C.c_void_p(df.data_ptr())) == _abi.TSDF_EINVAL
    # an empty box is fine, launches nothing and needs no buffer
    for hi in ([4, 0, 2], [0, 0, 0], [4, 3, 0]):
        e = i64(hi)
        pe = e.ctypes.data_as(_abi.L3)
        assert v._lib.tsdf_esdf_dense(v._ctx, pa, pe, 3, VS, 0.0, None, None) == _abi.TSDF_OK
        assert v._lib.tsdf_esdf_dense_device(v._ctx, pa, pe, 3, VS, 0.0, None,
                                             None) == _abi.TSDF_OK
    d, f = v.esdf([0, 0, 0], [4, 0, 2], 1.0)
    assert d.shape == (2, 0, 4) and f.shape == (2, 0, 4)
    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == 7.0).all() and (df.cpu().numpy() == 9).all()
    # the Python layer's radius rule
    for md in (0.0, -1.0, 128.5 * VS, nan):
        with pytest.raises(ValueError):
            v.esdf(*box, md)
    # one sector shard of two is refused, as sampling and raycasting are
    s = HipTSDFVolume(VS, TAU, n_sectors=2, sector=0, **SMALL)
    rc, d, f = host_call(s, *box, 3, VS, 0.0)
    assert rc == _abi.TSDF_EINVAL and "n_sectors > 1" in text(s) and text(s).startswith("esdf: ")
    assert np.isnan(d).all() and (f == 0xEE).all()
    s.close()


def test_esdf_around_pads_and_crops(maps, centre):
    from tsdf_map import box_around, esdf_around
    v = maps["vdbfusion_f64"]
    c = (centre + 0.5) * VS
    half = [1.0, 0.8, 0.4]
    md = max_dist(12)
    lo, hi = box_around(c, half, VS)
    g = esdf_around(v, c, half, md, pad=True)
    ref = er.of_volume(v, lo - 12, hi + 12, 12)
    crop = tuple(a[12:-12, 12:-12, 12:-12] for a in ref)
    assert g.lo.tolist() == lo.tolist() and g.hi.tolist() == hi.tolist()
    er.assert_same((g.dist, g.flags), crop)
    plain = esdf_around(v, c, half, md, pad=False)
    er.assert_same((plain.dist, plain.flags), er.of_volume(v, lo, hi, 12))
    # padding matters: somewhere the nearest surface lies outside the box
    assert not np.array_equal(er.bits(plain.dist), er.bits(g.dist))
    assert (np.abs(g.dist) <= np.abs(plain.dist)).all()
    assert g.clearance([c])[0] == g.dist[tuple((centre - lo)[::-1])]
