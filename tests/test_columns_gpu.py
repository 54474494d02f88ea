"""The column maps on the GPU (include/tsdf_hip_columns.h) against tests/colref.py, bit for bit:
floats as uint32, counts and flags as integers.  The reference reads the GPU volume's own
query_dense, so what test_columns_ref.py pins on the CPU is what the kernel is held to here.  Every
box goes through column_map, column_map_device and raw ctypes calls with subsets of NULL outputs."""
import ctypes as C

import numpy as np
import pytest

import colref as cr
import esdfref as er
import sampleref as sr

pytestmark = pytest.mark.gpu

F = np.float32
VS = sr.VOXEL_SIZE
TAU = sr.SDF_TRUNC
SMALL = dict(max_bricks=1 << 12, max_points=1 << 12, max_batch=4)
COL_WAVES, COL_GRID_CAP = 4, 8192   # columns_plan.h (tests/test_columns_plan.py pins them)
DTYPES = (F, F, np.uint16, np.uint16, np.uint8)
FILL = (7.0, 7.0, 0xABCD, 0xABCD, 0xEE)
SUBSETS = ((1, 0, 0, 0, 0), (0, 1, 0, 0, 1), (0, 0, 1, 1, 0), (0, 0, 0, 0, 1), (1, 1, 1, 1, 0))


def i64(a):
    return np.ascontiguousarray(np.asarray(a, np.int64).reshape(3))


def text(v):
    return v._lib.tsdf_last_error(v._ctx).decode()


def host_call(v, lo, hi, band=0.0, mw=0.0, mo=1, mf=1, use=(1, 1, 1, 1, 1)):
    """tsdf_column_map through ctypes: (rc, [five [y, x] arrays, pre-filled; None where unused])."""
    from tsdf_map import _abi
    lo, hi = i64(lo), i64(hi)
    n = np.maximum(hi - lo, 0)
    out = [np.full((n[1], n[0]), f, dt) if u else None for u, f, dt in zip(use, FILL, DTYPES)]
    types = (_abi.FP, _abi.FP, _abi.U16P, _abi.U16P, _abi.U8P)
    rc = v._lib.tsdf_column_map(v._ctx, lo.ctypes.data_as(_abi.L3), hi.ctypes.data_as(_abi.L3),
                                band, mw, mo, mf,
                                *[a.ctypes.data_as(t) if a is not None else None
                                  for a, t in zip(out, types)])
    return rc, out


def device_call(v, lo, hi, band=0.0, mw=0.0, mo=1, mf=1, use=(1, 1, 1, 1, 1)):
    """tsdf_column_map_device through ctypes into pre-filled tensors: (rc, tensors or None)."""
    import torch
    from tsdf_map import _abi
    lo, hi = i64(lo), i64(hi)
    n = np.maximum(hi - lo, 0)
    out = [torch.from_numpy(np.full((n[1], n[0]), f, dt)).to(v.tensor_device) if u else None
           for u, f, dt in zip(use, FILL, DTYPES)]
    torch.cuda.synchronize()
    rc = v._lib.tsdf_column_map_device(v._ctx, lo.ctypes.data_as(_abi.L3),
                                       hi.ctypes.data_as(_abi.L3), band, mw, mo, mf,
                                       *[C.c_void_p(t.data_ptr() if t is not None else 0)
                                         for t in out])
    return rc, out


def maps_of(m):
    return m.elev, m.ceil, m.n_occ, m.n_free, m.flags


def check_box(v, lo, hi, band=0.0, mw=0.0, mo=1, mf=1, ref=None, subsets=SUBSETS):
    """Both entry points, all outputs and subsets of them, against the reference; returns it."""
    from tsdf_map import _abi
    if ref is None:
        ref = cr.of_volume(v, lo, hi, band, mw, mo, mf)
    m = v.column_map(lo, hi, occ_band=band, min_weight=mw, min_occ=mo, min_free=mf)
    assert m.lo.tolist() == list(map(int, lo)) and m.hi.tolist() == list(map(int, hi))
    cr.assert_same(maps_of(m), ref)
    d = v.column_map_device(lo, hi, occ_band=band, min_weight=mw, min_occ=mo, min_free=mf)
    cr.assert_same([t.cpu().numpy() for t in d], ref)
    for k, use in enumerate(subsets):
        call = host_call if k % 2 == 0 else device_call
        rc, out = call(v, lo, hi, band, mw, mo, mf, use=use)
        assert rc == _abi.TSDF_OK, text(v)
        if call is device_call:
            out = [None if t is None else t.cpu().numpy() for t in out]
        assert [a is not None for a in out] == [bool(u) for u in use]
        cr.assert_same(out, ref)
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


@pytest.mark.parametrize("min_weight", [0.0, 2.0])
@pytest.mark.parametrize("band", [0.0, VS])
@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_fixture_box_bitwise(maps, fields, centre, sem, band, min_weight):
    lo, hi = er.fixture_box(centre)
    S, W = fields[sem]
    assert S.shape == (33, 80, 97)
    ref = cr.column_map(S, W, lo[2], VS, band, min_weight)
    c = cr.counts(S, W, min_weight, ref)
    print("%s band %g min_weight %g: %s" % (sem, band, min_weight, c))
    assert c["cells"] == 7760
    assert c["elev"] >= 2500 and c["free_only"] >= 300 and c["unobserved"] >= 1500
    assert c["ceil"] == 0  # the simulated scene has no ceiling
    check_box(maps[sem], lo, hi, band, min_weight, ref=ref)


def room_volume(lo):
    from tsdf_map import HipTSDFVolume
    S, W = cr.room(lo)
    v = HipTSDFVolume(VS, TAU, **SMALL)
    v.import_bricks(*cr.bricks_of(S, W, lo))
    hi = np.asarray(lo) + np.array(cr.ROOM_N)
    gs, gw = v.query_dense(lo, hi)  # the volume holds the field the room was built as
    assert np.array_equal(cr.bits(gs), cr.bits(S)) and np.array_equal(cr.bits(gw), cr.bits(W))
    return v, S, W, hi


def test_the_room_at_every_z_offset():
    """The room through import_bricks at lo z = -21 + k, k = 0..7: the chosen crossing pairs of both
    kinds straddle a z-brick boundary for some k, bricks between floor and ceiling are absent."""
    seen_up = seen_down = 0
    for k in range(8):
        lo = np.array([-13, 5, -21 + k])
        v, S, W, hi = room_volume(lo)
        for mw in (0.0, 2.0):
            ref = cr.column_map(S, W, lo[2], VS, 0.0, mw)
            c = cr.counts(S, W, mw, ref)
            u, d = cr.straddles(S, W, lo[2], mw)
            print(k, mw, c, (u, d))
            assert c["up2"] >= 30 and c["down2"] >= 30 and c["shelf"] >= 30
            seen_up += u
            seen_down += d
            check_box(v, lo, hi, 0.0, mw, ref=ref, subsets=SUBSETS[:2])
        check_box(v, lo, hi, VS, 0.0, 3, 2, subsets=())
        v.close()
    assert seen_up >= 100 and seen_down >= 100


def test_the_room_slab_between_floor_and_shelf():
    lo = np.array([-13, 5, -18])
    v, S, W, hi = room_volume(lo)
    a, b = lo.copy(), hi.copy()
    a[2], b[2] = lo[2] + cr.ROOM_SLAB[0], lo[2] + cr.ROOM_SLAB[1]
    ref = check_box(v, a, b, 0.0, 0.0, 1, 3)
    kinds = ref[4] & 7
    assert (kinds == cr.OBSERVED | cr.FREE).sum() >= 50 and (kinds == cr.OBSERVED).sum() >= 50
    assert (kinds == 0).sum() >= 20
    # a box cut out of the room's middle, at unaligned faces
    check_box(v, lo + [9, 3, 7], hi - [11, 6, 5], VS, 1.0, 2, 2)
    v.close()


def test_gridmap_helpers_on_the_room():
    from tsdf_map import ColumnMap, _abi, columns_around
    lo = np.array([-13, 5, -18])
    v, S, W, hi = room_volume(lo)
    ref = cr.column_map(S, W, lo[2], VS, 0.0, 0.0, 2, 2)
    m = v.column_map(lo, hi, min_occ=2, min_free=2)
    assert isinstance(m, ColumnMap) and m.voxel_size == VS
    elev, ceil, n_occ, n_free, flags = ref
    data, origin, res = m.occupancy_grid()
    want = np.where(n_occ >= 2, 100, np.where(n_free >= 2, 0, -1)).astype(np.int8)
    assert data.dtype == np.int8 and data.flags["C_CONTIGUOUS"] and np.array_equal(data, want)
    assert origin.tolist() == [lo[0] * VS, lo[1] * VS] and res == VS
    with np.errstate(invalid="ignore"):
        h = (ceil - elev).astype(F)
    assert np.array_equal(cr.bits(m.headroom()), cr.bits(h)) and (h < 0).sum() >= 30
    # step height: the largest |difference| to the 4-neighbours that have an elevation
    pad = np.pad(elev, 1, constant_values=np.nan)
    with np.errstate(invalid="ignore"):
        d = np.stack([np.abs(pad[1:-1, 1:-1] - pad[sl]) for sl in
                      ((slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1)),
                       (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None)))])
    none = np.isnan(d).all(0)
    step = np.where(none, np.nan, np.nanmax(np.where(none[None], 0, d), 0)).astype(F)
    got = m.step_height()
    assert np.array_equal(np.isnan(got), np.isnan(step))
    assert np.array_equal(got[~none], step[~none]) and (got[~none] > 2 * VS).sum() >= 20
    # columns_around: the box of esdf.box_around in x, y and of the heights in z
    c = (lo + np.array(cr.ROOM_N) // 2 + 0.5) * VS
    g = columns_around(v, c, [1.0, 0.7], c[2] - 0.9, c[2] + 0.4, occ_band=VS, min_free=2)
    blo = np.floor((c - [1.0, 0.7, 0]) / VS).astype(np.int64)
    bhi = np.floor((c + [1.0, 0.7, 0]) / VS).astype(np.int64) + 1
    assert g.lo[:2].tolist() == blo[:2].tolist() and g.hi[:2].tolist() == bhi[:2].tolist()
    assert g.lo[2] == np.floor((c[2] - 0.9) / VS) and g.hi[2] == np.floor((c[2] + 0.4) / VS) + 1
    cr.assert_same(maps_of(g), cr.of_volume(v, g.lo, g.hi, VS, 0.0, 1, 2))
    assert _abi.COLUMN_HAS_ELEV == cr.HAS_ELEV
    v.close()


SHAPES = [(1, 1, 1), (1, 1, 40), (97, 1, 5), (9, 9, 1), (67, 45, 21)]


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(maps, centre, shape):
    v = maps["vdbfusion_f64"]
    n = np.array(shape)
    lo = centre - n // 2   # (80, -51, -18) - ...: unaligned, negative in y and z
    if shape == (67, 45, 21):
        lo = np.array([-35, -73, -29])  # negative and unaligned on every axis
    ref = check_box(v, lo, lo + n, VS, 0.0, 2, 2)
    assert ref[0].shape == shape[1::-1]
    if shape == (1, 1, 1):
        assert cr.bits(ref[0])[0, 0] == 0x7FC00000 and cr.bits(ref[1])[0, 0] == 0x7FC00000
    if n.prod() > 400:
        assert (ref[4] & cr.OBSERVED != 0).sum() >= 10


def synthetic(voxels, sem="vdbfusion_f64"):
    from tsdf_map import HipTSDFVolume
    v = HipTSDFVolume(VS, TAU, semantics=sem, **SMALL)
    if voxels:
        v.import_bricks(*er.make_bricks(voxels, 0.0 if sem == "voxblox" else F(TAU)))
    return v


def test_an_absent_middle_brick_hides_the_crossings():
    """One column over three z-bricks, the middle one absent, the sign changing on either side of
    the gap: no crossing, whichever way the signs go."""
    for below, above in ((-0.1, 0.1), (0.1, -0.1)):
        vox = {(3, -2, z): (below, 1.0) for z in range(-8, 0)}
        vox.update({(3, -2, z): (above, 1.0) for z in range(8, 16)})
        v = synthetic(vox)
        for lo, hi in (([3, -2, -8], [4, -1, 16]), ([0, -8, -5], [8, 0, 13])):
            ref = check_box(v, lo, hi)
            col = tuple(np.array([-2, 3]) - np.array(lo)[1::-1])
            assert ref[4][col] == cr.OBSERVED | cr.OCCUPIED and np.isnan(ref[0]).all()
            assert ref[2][col] + ref[3][col] == min(hi[2], 16) - max(lo[2], -8) - 8
        v.close()
    # with the middle brick held (one observed voxel far from the column) and unobserved there, the
    # same; with the voxels next to the gap's faces joined, a crossing
    vox = {(3, -2, -1): (-0.1, 1.0), (3, -2, 0): (0.2, 1.0), (3, -2, 7): (0.1, 2.0),
           (3, -2, 8): (-0.3, 1.0)}
    v = synthetic(vox)
    ref = check_box(v, [0, -8, -8], [8, 0, 16])
    assert ref[4][6, 3] == 27 and ref[1][6, 3] > ref[0][6, 3]   # elev at z = 0, ceil at z = 8
    assert ref[0][6, 3] == ((F(0) + F(0.5)) - F(0.2) / (F(0.2) - F(-0.1))) * F(VS)
    v.close()


def test_absent_brick_columns_and_an_empty_map():
    v = synthetic({(100, 100, 100): (0.0, 1.0)})
    e = synthetic({})
    for vol in (v, e):
        for lo, hi in (([-3, -4, -5], [9, 3, 2]), ([0, 0, 0], [8, 8, 8]), ([-20, 1, -9], [-1, 2, 40])):
            ref = check_box(vol, lo, hi)
            assert (ref[4] == 0).all() and (ref[2] == 0).all() and (ref[3] == 0).all()
            assert (cr.bits(ref[0]) == 0x7FC00000).all() and (cr.bits(ref[1]) == 0x7FC00000).all()
    v.close()
    e.close()


def test_index_domain_edge():
    """Voxels at |i| >= 2^23 read unobserved; boxes straddle +-2^23 on x and on z and lie wholly
    outside, out to |i| near 2^50."""
    lim = 1 << 23
    vox = {(lim - 1, 2, -3): (-0.1, 1.0), (lim - 1, 2, -2): (0.1, 1.0),
           (-lim + 1, 0, 0): (0.1, 1.0), (-lim + 1, 0, 1): (-0.1, 1.0),
           (5, 6, -lim + 1): (-0.2, 1.0), (5, 6, -lim + 2): (0.1, 1.0),
           (5, 6, lim - 2): (0.2, 1.0), (5, 6, lim - 1): (-0.1, 1.0)}
    v = synthetic(vox)
    ref = check_box(v, [lim - 6, -2, -6], [lim + 7, 5, 3])  # straddles +2^23 on x
    assert ref[4][4, 5] == cr.OBSERVED | cr.OCCUPIED | cr.HAS_ELEV and (ref[4][:, 6:] == 0).all()
    assert ref[0][4, 5] == ((F(-2) + F(0.5)) - F(0.1) / (F(0.1) - F(-0.1))) * F(VS)
    ref = check_box(v, [-lim - 4, -2, -2], [-lim + 3, 3, 3])  # straddles -2^23 on x
    assert ref[4][2, 5] == cr.OBSERVED | cr.OCCUPIED | cr.HAS_CEIL and (ref[4][:, :5] == 0).all()
    ref = check_box(v, [3, 4, -lim - 5], [9, 9, -lim + 6])  # straddles -2^23 on z
    assert ref[4][2, 2] == cr.OBSERVED | cr.OCCUPIED | cr.HAS_ELEV
    assert ref[0][2, 2] == ((F(-lim + 2) + F(0.5)) - F(0.1) / (F(0.1) - F(-0.2))) * F(VS)
    ref = check_box(v, [3, 4, lim - 7], [9, 9, lim + 9])  # straddles +2^23 on z
    assert ref[4][2, 2] == cr.OBSERVED | cr.OCCUPIED | cr.HAS_CEIL
    assert ref[1][2, 2] == ((F(lim - 2) + F(0.5)) + F(0.2) / (F(0.2) - F(-0.1))) * F(VS)
    for lo, hi in (([lim, 0, 0], [lim + 9, 4, 3]), ([0, -lim - 9, 0], [3, -lim, 5]),
                   ([4, 5, lim], [7, 8, lim + 20]), ([4, 5, -lim - 20], [7, 8, -lim + 1]),
                   ([1 << 40, -(1 << 50), 0], [(1 << 40) + 5, -(1 << 50) + 6, 7]),
                   ([0, 0, (1 << 50) - 3], [9, 9, (1 << 50) + 14])):
        ref = check_box(v, lo, hi)  # wholly outside
        assert (ref[4] == 0).all() and (cr.bits(ref[0]) == 0x7FC00000).all()
    v.close()


def past_cap_case():
    """(voxels, lo, hi, seeded brick columns): the smallest square box with more than
    COL_GRID_CAP * COL_WAVES brick columns, 3 voxels tall across the z-brick boundary at z = 8,
    with crossings seeded in the brick columns on both sides of the trip boundary."""
    first = COL_GRID_CAP * COL_WAVES
    nb = int(np.ceil(np.sqrt(first + 1)))            # 182 brick columns a side
    n = 8 * (nb - 2) + 2                             # ... from one voxel of the first to one of the last
    lo = np.array([7, -1, 6])
    hi = lo + [n, n, 3]
    cols = [0, 1, first - 1, first, first + 1, first + COL_WAVES, nb * nb - 1]
    vox = {}
    for j, c in enumerate(cols):
        bx, by = lo[0] // 8 + c % nb, lo[1] // 8 + c // nb
        for dx, dy in ((0, 0), (7, 0), (3, 7), (7, 7)):
            x, y = int(bx * 8 + dx), int(by * 8 + dy)
            up = (j + dx + dy) % 2 == 0
            vox[(x, y, 7)] = (-0.1 if up else 0.2, 1.0)
            vox[(x, y, 8)] = (0.15 if up else -0.05, 2.0)
    return vox, lo, hi, nb, cols


def test_past_the_grid_cap():
    first = COL_GRID_CAP * COL_WAVES
    vox, lo, hi, nb, cols = past_cap_case()
    n = hi - lo
    assert nb == 182 and nb * nb > first >= (nb - 1) ** 2 and int(n.prod()) < 1 << 23
    assert (lo[0] + n[0] - 1) // 8 - lo[0] // 8 + 1 == nb == (lo[1] + n[1] - 1) // 8 - lo[1] // 8 + 1
    # the restated mapping (tests/test_columns_plan.py): groups of COL_WAVES columns, workgroup
    # g % grid on trip g // grid; the seeded columns lie in the last group of trip 0 and the first
    # of trip 1
    trip = lambda c: (c // COL_WAVES) // COL_GRID_CAP   # noqa: E731
    assert [trip(c) for c in cols] == [0, 0, 0, 1, 1, 1, 1]
    v = synthetic(vox)
    ref = check_box(v, lo, hi, subsets=SUBSETS[:2])
    seeded = ref[4] != 0
    # every seeded voxel pair inside the box shows as a crossing, on both sides of the boundary
    inside = [(x, y) for (x, y, z) in vox if z == 7 and lo[0] <= x < hi[0] and lo[1] <= y < hi[1]]
    assert seeded.sum() == len(inside) >= 4 * (len(cols) - 2)
    for kind in (cr.HAS_ELEV, cr.HAS_CEIL):
        for t in (0, 1):
            hit = [(x, y) for x, y in inside
                   if ref[4][y - lo[1], x - lo[0]] & kind
                   and trip((x // 8 - lo[0] // 8) + nb * (y // 8 - lo[1] // 8)) == t]
            assert len(hit) >= 2, (kind, t)
    v.close()


def test_two_calls_give_the_same_bits_and_leave_the_map(maps, centre):
    v = maps["voxblox"]
    lo, hi = er.fixture_box(centre)
    before = v.export_voxels()
    a = maps_of(v.column_map(lo, hi, occ_band=VS))
    b = maps_of(v.column_map(lo, hi, occ_band=VS))
    cr.assert_same(a, b)
    d = v.column_map_device(lo, hi, occ_band=VS)
    cr.assert_same([t.cpu().numpy() for t in d], a)
    after = v.export_voxels()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(cr.bits(before[1]), cr.bits(after[1]))


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
    check_box(g, lo, hi, subsets=SUBSETS[:1])  # (flushes the pending batch itself)
    g.integrate(*scans[1])
    o.integrate(*scans[1])
    gv, ov = g.export_voxels(), o.export_voxels()
    assert np.array_equal(gv[0], ov[0])
    assert np.array_equal(cr.bits(gv[1]), cr.bits(ov[1]))
    assert np.array_equal(cr.bits(gv[2]), cr.bits(ov[2]))
    g.close()
    o.close()


def test_after_evict_and_after_growth(scan0, centre):
    from tsdf_map import HipTSDFVolume
    pts = np.ascontiguousarray(scan0[0][::4])
    lo, hi = er.fixture_box(centre)
    # growth: pool and table are reallocated while the map is built
    g = HipTSDFVolume(VS, TAU, max_bricks=128)
    g.integrate(pts, scan0[1])
    g.sync()
    st = g.stats()
    assert st["n_grows"] >= 1 and st["n_bricks"] > 128
    ref = check_box(g, lo, hi, VS, subsets=SUBSETS[:1])
    assert (ref[4] & cr.HAS_ELEV != 0).sum() >= 500 and (ref[4][:11] != 0).any()
    # evict: the bricks outside a brick box that cuts the fixture box go, the pool is compacted
    blo, bhi = (lo >> 3) + [3, 2, 0], (hi >> 3) - [2, 3, 0]
    assert g.evict_outside(blo, bhi, copy_out=False) > 0
    after = check_box(g, lo, hi, VS, subsets=SUBSETS[:1])
    assert not np.array_equal(after[4], ref[4]) and (after[4] & cr.HAS_ELEV != 0).sum() >= 100
    ylim, xlim = int(blo[1] * 8 - lo[1]), int(blo[0] * 8 - lo[0])
    assert ylim > 8 and xlim > 8 and (after[4][:ylim] == 0).all() and (after[4][:, :xlim] == 0).all()
    g.close()


def test_refusals(maps):
    import torch
    from tsdf_map import HipTSDFVolume, _abi
    v = maps["vdbfusion_f64"]
    nan, inf = float("nan"), float("inf")
    box = ([0, 0, 0], [4, 3, 2])
    ok = (0.0, 0.0, 1, 1)
    bad = [
        (*box, nan, 0.0, 1, 1, "occ_band is not finite"),
        (*box, inf, 0.0, 1, 1, "occ_band is not finite"),
        (*box, -inf, -1.0, 0, 0, "occ_band is not finite"),
        (*box, 0.0, -1.0, 1, 1, "min_weight is negative or NaN"),
        (*box, 0.0, nan, 0, 1, "min_weight is negative or NaN"),
        (*box, 0.0, 0.0, 0, 1, "min_occ and min_free must be in 1..65535"),
        (*box, 0.0, 0.0, 1, 65536, "min_occ and min_free must be in 1..65535"),
        ([0, 0, 0], [4, -1, 2], 0.0, 0.0, 1, 0, "min_occ and min_free must be in 1..65535"),
        ([0, 0, 0], [4, -1, 2], *ok, "hi < lo"),
        ([0, 0, 0], [4, -1, 1 << 31], *ok, "hi < lo"),
        ([0, 0, 0], [4, 1 << 31, 2], *ok, "box extent >= 2^31 voxels"),
        ([-(1 << 62), 0, 0], [1 << 62, 1, 1], *ok, "box extent >= 2^31 voxels"),
        ([0, 0, 0], [1 << 14, 1 << 14, 65536], *ok, "box above 65535 voxels in z"),
        ([0, 0, 0], [4, 3, 65536], *ok, "box above 65535 voxels in z"),
        ([0, 0, 0], [(1 << 13) + 1, 1 << 13, 2], *ok, "box above 2^26 columns"),
    ]
    for lo, hi, band, mw, mo, mf, msg in bad:
        for call in (host_call, device_call):
            rc, out = refused(v, call, lo, hi, band, mw, mo, mf)
            assert rc == _abi.TSDF_EINVAL and text(v) == "columns: " + msg, (lo, hi, text(v))
            untouched(out)
    # NULL arguments: the bounds, and all five outputs for a box that is not empty
    a, b = i64(box[0]), i64(box[1])
    pa, pb = a.ctypes.data_as(_abi.L3), b.ctypes.data_as(_abi.L3)
    none = (None,) * 5
    for fn in (v._lib.tsdf_column_map, v._lib.tsdf_column_map_device):
        assert fn(v._ctx, None, pb, *ok, *none) == _abi.TSDF_EINVAL
        assert text(v) == "columns: null argument"
        assert fn(v._ctx, pa, None, *ok, *none) == _abi.TSDF_EINVAL
        assert fn(v._ctx, pa, pb, *ok, *none) == _abi.TSDF_EINVAL
        assert text(v) == "columns: null buffer"
        # an empty box is fine, launches nothing and needs no buffer
        for hi in ([4, 0, 2], [0, 0, 0], [4, 3, 0], [0, 3, 70000]):
            e = i64(hi)
            assert fn(v._ctx, pa, e.ctypes.data_as(_abi.L3), *ok, *none) == _abi.TSDF_OK
    m = v.column_map([0, 0, 0], [4, 0, 2])
    assert m.elev.shape == (0, 4) and m.flags.shape == (0, 4)
    torch.cuda.synchronize()
    # one sector shard of two is refused, as sampling and raycasting are
    s = HipTSDFVolume(VS, TAU, n_sectors=2, sector=0, **SMALL)
    for call in (host_call, device_call):
        rc, out = call(s, *box)
        assert rc == _abi.TSDF_EINVAL and "n_sectors > 1" in text(s)
        assert text(s).startswith("columns: ")
        untouched(out)
    s.close()


def refused(v, call, lo, hi, band, mw, mo, mf):
    """A call that must be refused, into pre-filled buffers of 24 cells whatever the box says."""
    import torch
    from tsdf_map import _abi
    lo, hi = i64(lo), i64(hi)
    out = [np.full(24, f, dt) for f, dt in zip(FILL, DTYPES)]
    pl, ph = lo.ctypes.data_as(_abi.L3), hi.ctypes.data_as(_abi.L3)
    if call is host_call:
        types = (_abi.FP, _abi.FP, _abi.U16P, _abi.U16P, _abi.U8P)
        rc = v._lib.tsdf_column_map(v._ctx, pl, ph, band, mw, mo, mf,
                                    *[a.ctypes.data_as(t) for a, t in zip(out, types)])
        return rc, out
    dev = [torch.from_numpy(a).to(v.tensor_device) for a in out]
    torch.cuda.synchronize()
    rc = v._lib.tsdf_column_map_device(v._ctx, pl, ph, band, mw, mo, mf,
                                       *[C.c_void_p(t.data_ptr()) for t in dev])
    torch.cuda.synchronize()
    return rc, dev


def untouched(out):
    for a, f, dt in zip(out, FILL, DTYPES):
        if a is None:
            continue
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        assert a.dtype == dt and (a == dt(f)).all()
