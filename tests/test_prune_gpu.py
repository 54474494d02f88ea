"""Prune and evict on the GPU (include/tsdf_hip_prune.h).

The oracle cannot remove bricks, so the reference is its own export filtered in numpy: integrate A
into an oracle volume, export, keep or drop rows by brick coordinate (or voxels by weight), import
the kept rows into a fresh oracle volume (an import into empty bricks is a plain copy), integrate
B, and compare `export_voxels` bit for bit.  The slot patterns run on imported synthetic bricks
whose values are a function of (brick, voxel): there the reference is the GPU's own export before
the call, filtered."""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import decimate

pytestmark = pytest.mark.gpu

VS, TAU = 0.05, 0.15
BLOCK = 256                     # slots per block of the keep scan (tsdf_device.h RM_BLOCK)
BMIN, BMAX = -(1 << 20), 1 << 20
ALL = ([BMIN] * 3, [BMAX] * 3)  # the box holding every packable brick


def hip(**kw):
    from tsdf_map import HipTSDFVolume
    kw.setdefault("max_bricks", 1 << 16)
    return HipTSDFVolume(kw.pop("voxel_size", VS), kw.pop("sdf_trunc", TAU), **kw)


def ora(**kw):
    for k in ("max_batch", "pipeline", "max_bricks"):
        kw.pop(k, None)
    return oracle.OracleTSDFVolume(kw.pop("voxel_size", VS), kw.pop("sdf_trunc", TAU), **kw)


def sem_kw(semantics, **kw):
    kw.update(semantics=semantics)
    if semantics == "voxblox":
        kw.update(max_range=40.0)
    return kw


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_voxels(a, b):
    (ai, as_, aw), (bi, bs, bw) = a, b
    return (ai.shape == bi.shape and np.array_equal(ai, bi) and np.array_equal(aw, bw)
            and np.array_equal(bits(as_), bits(bs)))


def bitwise(g, o):
    return same_voxels(g.export_voxels(), o.export_voxels())


def same_bricks(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
            and np.array_equal(bits(a[2]), bits(b[2])))


def inside(coords, lo, hi):
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    return np.all((c >= np.asarray(lo)) & (c < np.asarray(hi)), axis=1)


def rows(bricks, mask):
    return tuple(x[mask] for x in bricks)


def reference(o, keep_mask_of, then=(), **kw):
    """The reference method: o's export filtered by keep_mask_of(coords), imported into a fresh
    oracle volume, then the scans of `then` integrated."""
    pre = o.export_bricks()
    o2 = ora(**kw)
    o2.import_bricks(*rows(pre, keep_mask_of(pre[0])))
    for pts, org in then:
        o2.integrate(pts, org)
    return o2


def synthetic(n):
    """n bricks on a line through negative and positive coordinates, values a function of
    (brick, voxel); brick i has y = i & 1, so a box on y takes every second one."""
    i = np.arange(n, dtype=np.int64)
    t = i - n // 2
    coords = np.stack([t, i & 1, -t], 1).astype(np.int32)
    v = np.arange(512, dtype=np.float32)
    sdf = (i[:, None].astype(np.float32) * np.float32(0.001) + v[None, :] / np.float32(4096))
    w = (1 + (i[:, None] % 7) + (np.arange(512)[None, :] % 3)).astype(np.float32)
    w[:, 5::11] = 0  # unobserved voxels inside observed bricks
    return coords, np.ascontiguousarray(sdf, np.float32), w


def in_two_calls(n, n1):
    """A volume holding synthetic(n): bricks [0, n1) imported first (the low pool slots), the
    rest second (the high ones)."""
    c, s, w = synthetic(n)
    g = hip(max_bricks=max(1 << 12, 2 * n))
    if n1:
        g.import_bricks(c[:n1], s[:n1], w[:n1])
    if n1 < n:
        g.import_bricks(c[n1:], s[n1:], w[n1:])
    assert g.num_bricks() == n
    return g, c


def evict_and_check(g, lo, hi):
    """One eviction against the filtered pre-export, with every check of the issue's list."""
    pre = g.export_bricks()
    keep = inside(pre[0], lo, hi)
    assert g.count_outside(lo, hi) == int((~keep).sum())
    ev = g.evict_outside(lo, hi)
    assert same_bricks(ev, rows(pre, ~keep))        # (z, y, x) order: the export's, filtered
    assert same_bricks(g.export_bricks(), rows(pre, keep))
    assert g.num_bricks() == g.stats()["n_bricks"] == int(keep.sum())
    assert g.count_outside(lo, hi) == 0
    bg = np.float32(0.0 if g.semantics == "voxblox" else g.sdf_trunc)
    gone = pre[0][~keep]
    for b in gone[[0, len(gone) // 2, -1]] if len(gone) else ():
        b = b.astype(np.int64)
        s, w = g.query_dense(8 * b, 8 * b + 8)
        assert np.all(w == 0) and np.all(bits(s) == bits(bg))
        p = ((8 * b + 4) * np.float64(g.voxel_size)).reshape(1, 3)
        assert not g.sample(p, mode="nearest")[3][0]
    return ev


N_SLOTS = 3 * BLOCK + 37
N1 = BLOCK + 19


@pytest.mark.parametrize("pattern", ["set1", "set2", "second", "all", "none"])
def test_slot_patterns(pattern, scan0):
    g, c = in_two_calls(N_SLOTS, N1)
    split = int(c[N1, 0])  # x of the first brick of set 2 (x grows with the brick index)
    lo, hi = {
        "set1": ([split, BMIN, BMIN], [BMAX] * 3),      # every hole in the head: the most moves
        "set2": ([BMIN] * 3, [split, BMAX, BMAX]),      # the tail only: nothing moves
        "second": ([BMIN, 0, BMIN], [BMAX, 1, BMAX]),   # every second brick
        "all": ([0, 0, 0], [0, 0, 0]),                  # an empty box
        "none": ALL,
    }[pattern]
    pre = g.export_bricks()
    ev = evict_and_check(g, lo, hi)
    want = {"set1": N1, "set2": N_SLOTS - N1, "second": N_SLOTS // 2, "all": N_SLOTS, "none": 0}
    assert len(ev[0]) == want[pattern]
    # the map still takes imports: with the evicted bricks back it is what it was
    g.import_bricks(*ev)
    assert same_bricks(g.export_bricks(), pre)
    if pattern == "all":
        g2 = hip()
        g2.import_bricks(*synthetic(3))
        g2.evict_outside([0, 0, 0], [0, 0, 0], copy_out=False)
        assert g2.num_bricks() == 0
        pts = decimate(scan0[0], 16)
        g2.integrate(pts, scan0[1])
        o = ora()
        o.integrate(pts, scan0[1])
        assert bitwise(g2, o)


def test_one_brick():
    for box, n_ev in ((ALL, 0), (([0, 0, 0], [0, 0, 0]), 1)):
        g, _ = in_two_calls(1, 1)
        assert len(evict_and_check(g, *box)[0]) == n_ev
    g, _ = in_two_calls(1, 1)
    assert g.evict_outside([0, 0, 0], [0, 0, 0], copy_out=False) == 1 and g.num_bricks() == 0
    assert g.evict_outside([0, 0, 0], [0, 0, 0], copy_out=False) == 0  # an empty map


def test_scan_carries_between_rounds():
    """The scan's middle phase takes the block sums 64 at a time and carries from one round to the
    next: 64 * BLOCK + ... bricks need two rounds, and a removed brick in every block makes every
    carry matter."""
    n = 64 * BLOCK + BLOCK + 5
    g, c = in_two_calls(n, n // 3)
    pre = g.export_bricks()
    lo, hi = [BMIN, 0, BMIN], [BMAX, 1, BMAX]
    keep = inside(pre[0], lo, hi)
    assert g.count_outside(lo, hi) == n // 2
    ev = g.evict_outside(lo, hi)
    assert same_bricks(ev, rows(pre, ~keep))
    assert same_bricks(g.export_bricks(), rows(pre, keep))
    # and the tail of the line removed from what is left
    x_cut = int(c[n - 3 * BLOCK, 0])
    evict_and_check(g, [BMIN] * 3, [x_cut, BMAX, BMAX])


def test_box_is_half_open_down_to_the_lowest_brick():
    from tsdf_map import TsdfError, _abi
    cs = np.array([[-1, -1, -1], [0, 0, 0], [BMIN, -1, 0], [BMIN, BMIN, BMIN], [3, -1, 2],
                   [BMAX - 1, 0, -1], [2, 2, 2]], np.int32)
    c0, s0, w0 = synthetic(len(cs))
    g = hip()
    g.import_bricks(cs, s0, w0)
    # a brick at lo is kept, a brick at hi is removed
    ev = evict_and_check(g, [BMIN, BMIN, BMIN], [3, 2, 3])
    assert sorted(map(tuple, ev[0])) == sorted([(3, -1, 2), (BMAX - 1, 0, -1), (2, 2, 2)])
    ev = evict_and_check(g, [-1, -1, -1], [BMAX] * 3)
    assert sorted(map(tuple, ev[0])) == sorted([(BMIN, -1, 0), (BMIN, BMIN, BMIN)])
    assert g.num_bricks() == 2
    ev = evict_and_check(g, [-1, -1, -1], [0, 0, 0])
    assert [tuple(r) for r in ev[0]] == [(0, 0, 0)]
    with pytest.raises(ValueError):
        g.evict_outside([1, 0, 0], [0, 5, 5])
    lo, hi = (C.c_int32 * 3)(1, 0, 0), (C.c_int32 * 3)(0, 5, 5)
    n = C.c_uint64()
    assert g._lib.tsdf_count_outside(g._ctx, lo, hi, C.byref(n)) == _abi.TSDF_EINVAL
    assert g._lib.tsdf_evict_outside(g._ctx, lo, hi, None, None, None, 0,
                                     C.byref(n)) == _abi.TSDF_EINVAL
    with pytest.raises(TsdfError):
        g.prune(-1.0)
    with pytest.raises(TsdfError):
        g.prune(float("nan"))
    assert g.num_bricks() == 1


@pytest.fixture(scope="module")
def scans(sim):
    """Scans 0..3 of the trajectory, every fourth point."""
    return [(decimate(p, 4), o) for p, o in (sim.scan(k) for k in range(4))]


def cut_box(coords):
    """A box that cuts through the bricks of `coords`: everything below their median x."""
    c = np.asarray(coords, np.int64)
    lo, hi = c.min(0), c.max(0) + 1
    hi[0] = int(np.median(c[:, 0]))
    return lo, hi


def test_round_trip(scans):
    g, o = hip(), ora()
    for pts, org in scans[:2]:
        g.integrate(pts, org)
        o.integrate(pts, org)
    lo, hi = cut_box(o.export_bricks()[0])
    ev = g.evict_outside(lo, hi)
    assert len(ev[0]) and g.num_bricks()
    assert not bitwise(g, o)
    g.import_bricks(*ev)
    assert bitwise(g, o)


@pytest.mark.parametrize("pipeline", [False, True, 2])
@pytest.mark.parametrize("semantics", ["vdbfusion_f64", "vdbfusion", "voxblox"])
def test_evict_then_integrate_into_the_removed_region(scans, semantics, pipeline):
    """Freed slots not refilled, stale touched / cell entries under a rebuilt table or a bad rehash
    all show here: the scans come back to the removed region (Voxblox: background 0, not tau)."""
    kw = sem_kw(semantics)
    g, o = hip(max_batch=2, pipeline=pipeline, **kw), ora(**kw)
    for pts, org in scans:
        g.integrate(pts, org)
        o.integrate(pts, org)
    lo, hi = cut_box(o.export_bricks()[0])
    n0 = g.num_bricks()
    n_ev = g.evict_outside(lo, hi, copy_out=False)
    assert 0 < n_ev < n0 and g.num_bricks() == n0 - n_ev
    again = [scans[1], scans[3], scans[0]]
    for pts, org in again:
        g.integrate(pts, org)
    assert bitwise(g, reference(o, lambda c: inside(c, lo, hi), again, **kw))


def test_growth_after_eviction(scans, scan0):
    g, o = hip(max_bricks=128, max_batch=2), ora()
    first = (decimate(scan0[0], 32), scan0[1])
    g.integrate(*first)
    o.integrate(*first)
    g.sync()
    grows = g.stats()["n_grows"]
    assert grows >= 1
    c = o.export_bricks()[0]
    mid = np.median(c, 0).astype(np.int64)  # most of the map goes
    lo, hi = np.array([mid[0] - 3, mid[1] - 3, c[:, 2].min()]), np.array([mid[0] + 3, mid[1] + 3,
                                                                          c[:, 2].max() + 1])
    n0 = g.num_bricks()
    assert g.evict_outside(lo, hi, copy_out=False) > n0 // 2
    for pts, org in scans:
        g.integrate(pts, org)
    g.sync()
    st = g.stats()
    assert st["n_grows"] > grows
    o2 = reference(o, lambda c: inside(c, lo, hi), scans)
    assert bitwise(g, o2) and st["n_bricks"] == o2.num_bricks()


def test_overflow_leaves_the_map_alone(scans):
    from tsdf_map import _abi
    g = hip()
    g.integrate(*scans[0])
    pre = g.export_bricks()
    lo, hi = cut_box(pre[0])
    blo = (C.c_int32 * 3)(*[int(x) for x in lo])
    bhi = (C.c_int32 * 3)(*[int(x) for x in hi])
    count = g.count_outside(lo, hi)
    assert count > 1
    coords = np.full((count, 3), 77, np.int32)
    n = C.c_uint64()
    rc = g._lib.tsdf_evict_outside(g._ctx, blo, bhi, coords.ctypes.data_as(_abi.I3), None, None,
                                   count - 1, C.byref(n))
    assert rc == _abi.TSDF_EOVERFLOW and n.value == count
    assert np.all(coords == 77)
    assert same_bricks(g.export_bricks(), pre) and g.num_bricks() == len(pre[0])
    # coords alone, then the rest is gone
    rc = g._lib.tsdf_evict_outside(g._ctx, blo, bhi, coords.ctypes.data_as(_abi.I3), None, None,
                                   count, C.byref(n))
    assert rc == _abi.TSDF_OK and n.value == count
    assert np.array_equal(coords, pre[0][~inside(pre[0], lo, hi)])
    assert same_bricks(g.export_bricks(), rows(pre, inside(pre[0], lo, hi)))


@pytest.fixture(scope="module")
def three_scans(scans):
    """Three overlapping scans on both sides: (the GPU's bricks, the oracle volume)."""
    g, o = hip(), ora()
    for pts, org in scans[:3]:
        g.integrate(pts, org)
        o.integrate(pts, org)
    return g.export_bricks(), o


@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_prune(three_scans, m):
    bricks, o = three_scans
    g = hip()
    g.import_bricks(*bricks)  # (into empty bricks: a plain copy)
    n0 = g.num_bricks()
    removed = g.prune(m)
    oi, os_, ow = o.export_voxels()
    live = (ow >= m) & (ow > 0)
    assert 0 < live.sum() and (m < 2 or live.sum() < len(ow))
    assert same_voxels(g.export_voxels(), (oi[live], os_[live], ow[live]))
    nb = len(np.unique(oi[live].astype(np.int64) >> 3, axis=0))
    assert g.num_bricks() == nb == g.stats()["n_bricks"] and removed == n0 - nb
    if m >= 2:
        assert removed > 0
    # the reset voxels read as background
    c, s, w = g.export_bricks()
    bg = np.float32(TAU)
    assert np.all(bits(s[w == 0]) == bits(bg))
    assert g.prune(m) == 0 and same_bricks(g.export_bricks(), (c, s, w))


@pytest.mark.parametrize("semantics", ["vdbfusion_f64", "voxblox"])
def test_prune_then_integrate(scans, semantics):
    kw = sem_kw(semantics)
    g, o = hip(max_batch=2, **kw), ora(**kw)
    for pts, org in scans[:3]:
        g.integrate(pts, org)
        o.integrate(pts, org)
    c, s, w = o.export_bricks()
    m = np.float32(2.0) if semantics != "voxblox" else np.float32(np.median(w[w > 0]))
    bg = np.float32(0.0 if semantics == "voxblox" else TAU)
    s, w = s.copy(), w.copy()
    s[w < m] = bg
    w[w < m] = 0
    keep = (w > 0).reshape(len(c), -1).any(1)
    assert 0 < keep.sum() < len(c)
    o2 = ora(**kw)
    o2.import_bricks(c[keep], s[keep], w[keep])
    assert g.prune(float(m)) == len(c) - keep.sum()
    assert g.num_bricks() == keep.sum()
    for pts, org in (scans[1], scans[3]):
        g.integrate(pts, org)
        o2.integrate(pts, org)
    assert bitwise(g, o2)


def test_mesh_after_eviction(scans):
    g, o = hip(), ora()
    for pts, org in scans[:2]:
        g.integrate(pts, org)
        o.integrate(pts, org)
    lo, hi = cut_box(o.export_bricks()[0])
    assert g.evict_outside(lo, hi, copy_out=False) > 0
    o2 = reference(o, lambda c: inside(c, lo, hi))
    vg, _ = g.extract_triangle_mesh()
    vo, _ = o2.extract_triangle_mesh()
    assert len(vo) and vg.shape == vo.shape and np.array_equal(bits(vg), bits(vo))


@pytest.mark.parametrize("semantics", ["vdbfusion_f64", "vdbfusion"])
def test_sliding_window(sim, semantics, tmp_path):
    """Twelve scans out along the trajectory and back (6 m of arc), a 5 m window evicted after
    every scan: bricks leave, are seen again and leave again (the far wall after every scan, the
    ground as the sensor returns), and the bricks between the turning points never leave."""
    from tsdf_map import NpzArchive, SlidingWindow
    ks = [0, 30, 60, 30, 0, 30, 60, 30, 0, 30, 60, 30]
    kw = sem_kw(semantics)
    g, o = hip(max_batch=2, **kw), ora(**kw)
    win = SlidingWindow(g, 5.0, every=1, archive=NpzArchive(tmp_path / "parts"))
    peak = 0
    for k in ks:
        pts, org = sim.scan(k)
        pts = decimate(pts, 8)
        win.integrate(pts, org)
        o.integrate(pts, org)
        peak = max(peak, g.num_bricks())
    assert peak < o.num_bricks()  # the live map stays below the never-evicted one
    parts = list(win.archive)
    assert len(parts) == len(ks)
    keys = np.concatenate([p[0] for p in parts]).astype(np.int64)
    uniq, cnt = np.unique(keys, axis=0, return_counts=True)
    assert cnt.max() >= 2  # a brick evicted, seen again and evicted again
    full = win.full_map()
    gi, gs, gw = full.export_voxels()
    oi, os_, ow = o.export_voxels()
    assert np.array_equal(gi, oi) and np.array_equal(gw, ow)
    def packed(b):
        b = b.astype(np.int64) + BMAX
        return b[:, 0] | (b[:, 1] << 21) | (b[:, 2] << 42)
    never = ~np.isin(packed(oi.astype(np.int64) >> 3), packed(uniq))
    assert never.any() and not never.all()
    assert np.array_equal(bits(gs[never]), bits(os_[never]))
    err = np.abs(gs.astype(np.float64) - os_.astype(np.float64))
    print("sliding window %s: max |dS| %.3g m over %d merged voxels" %
          (semantics, err[~never].max(), (~never).sum()))
    assert err[~never].max() <= 1e-5
