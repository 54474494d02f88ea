"""The frontier voxels on the GPU (include/tsdf_hip_frontier.h) against tests/frontierref.py, bit for
bit: every output as integers, and the counts.  The reference reads the GPU volume's own
query_dense (a box) or export_bricks (the whole map), so what test_frontier_ref.py pins on the CPU
is what the kernels are held to here.  Every case goes through frontiers, frontiers_device and raw
ctypes calls with n_unknown / dir NULL in turn."""
import ctypes as C

import numpy as np
import pytest

import frontierref as fr
import sampleref as sr

pytestmark = pytest.mark.gpu

F = np.float32
VS = sr.VOXEL_SIZE
TAU = sr.SDF_TRUNC
SMALL = dict(max_bricks=1 << 12, max_points=1 << 12, max_batch=4)
GRID_CAP = 2048  # frontier_plan.h (tests/test_frontier_plan.py pins it)
B20 = 1 << 20
KNOWN = {6: (1, 2, 3), 18: (5, 9, 12), 26: (9, 15, 19)}
NAMES = ("tsdf_frontier_count", "tsdf_frontier_voxels", "tsdf_frontier_voxels_device")
ZERO = {"n_bricks": 0, "n_frontier_bricks": 0, "n_voxels": 0, "n_free": 0}
# the box of the integrated-map test: chosen on the CPU from the oracle's field of the same scan
# (bit-identical to the GPU's); not brick-aligned, 93 x 90 x 61 voxels
SCAN_LO, SCAN_HI = (3, -45, -21), (96, 45, 40)


def i64(a):
    return np.ascontiguousarray(np.asarray(a, np.int64).reshape(3))


def text(v):
    return v._lib.tsdf_last_error(v._ctx).decode()


def raw(v, name, lo=None, hi=None, band=VS, mw=0.0, conn=6, mu=1, cap=0, use=(1, 1, 1)):
    """An entry point through ctypes into buffers of cap voxels pre-filled with 0x5A bytes:
    (rc, counts dict, [coords, n_unknown, dir] as numpy or None where unused)."""
    import torch
    from tsdf_map import _abi
    plo = None if lo is None else i64(lo).ctypes.data_as(_abi.L3)
    phi = None if hi is None else i64(hi).ctypes.data_as(_abi.L3)
    st = _abi.FrontierCounts(77, 77, 77, 77)
    fn = getattr(v._lib, name)
    head = (v._ctx, plo, phi, band, mw, conn, mu)
    if name == "tsdf_frontier_count":
        return fn(*head, C.byref(st)), st.as_dict(), None
    shapes = (((cap, 3), np.int32), ((cap,), np.uint8), ((cap, 3), np.int8))
    out = [np.empty(s, dt) if u else None for (s, dt), u in zip(shapes, use)]
    for a in out:
        if a is not None:
            a.view(np.uint8)[...] = 0x5A
    if name == "tsdf_frontier_voxels":
        types = (_abi.I3, _abi.U8P, _abi.I8P)
        rc = fn(*head, *[a.ctypes.data_as(t) if a is not None else None
                         for a, t in zip(out, types)], cap, C.byref(st))
        return rc, st.as_dict(), out
    dev = [torch.from_numpy(a).to(v.tensor_device) if a is not None else None for a in out]
    torch.cuda.synchronize()
    rc = fn(*head, *[C.c_void_p(t.data_ptr() if t is not None else 0) for t in dev], cap,
            C.byref(st))
    return rc, st.as_dict(), [t.cpu().numpy() if t is not None else None for t in dev]


def n_bricks_of(v, lo, hi):
    """The held bricks that intersect the box (None: all of them)."""
    c = v.brick_coords().astype(np.int64) * 8
    if lo is None:
        return c.shape[0]
    lo, hi = i64(lo), i64(hi)
    if np.any(hi <= lo):
        return 0
    return int(np.all((c + 8 > lo) & (c < hi), axis=1).sum())


def check(v, lo=None, hi=None, band=VS, mw=0.0, conn=6, mu=1, ref=None):
    """All three entry points against the reference (dense for a box, sparse without); returns it."""
    from tsdf_map import _abi
    if ref is None:
        ref = (fr.of_bricks(v, band, mw, conn, mu) if lo is None
               else fr.of_volume(v, lo, hi, band, mw, conn, mu))
    if ref.counts["n_bricks"] is None:
        ref.counts["n_bricks"] = n_bricks_of(v, lo, hi)
    kw = dict(free_band=band, min_weight=mw, connectivity=conn, min_unknown=mu)
    s = v.frontiers(lo, hi, **kw)
    fr.assert_same((s.coords, s.n_unknown, s.dir), ref, s.counts)
    assert s.voxel_size == v.voxel_size
    assert v.frontier_counts(lo, hi, **kw) == ref.counts
    dc, dn, dd, counts = v.frontiers_device(lo, hi, **kw)
    assert dc.device.type == "cuda"
    fr.assert_same((dc.cpu().numpy(), dn.cpu().numpy(), dd.cpu().numpy()), ref, counts)
    n = ref.counts["n_voxels"]
    for name, use in (("tsdf_frontier_voxels", (1, 0, 1)), ("tsdf_frontier_voxels_device", (1, 1, 0)),
                      ("tsdf_frontier_voxels", (1, 1, 0)), ("tsdf_frontier_voxels_device", (1, 0, 0))):
        rc, st, out = raw(v, name, lo, hi, band, mw, conn, mu, cap=n + 2, use=use)
        assert rc == _abi.TSDF_OK, text(v)
        assert [a is not None for a in out] == [bool(u) for u in use]
        fr.assert_same([a[:n] if a is not None else None for a in out], ref, st)
        for a in out:  # nothing is written past the last frontier voxel
            assert a is None or np.all(a[n:].view(np.uint8) == 0x5A)
    return ref


def volume(bricks, **kw):
    """A small volume holding {(bx, by, bz): (S, W)} (scalars or 8^3 [z, y, x] arrays)."""
    from tsdf_map import HipTSDFVolume
    v = HipTSDFVolume(VS, TAU, **{**SMALL, **kw})
    if bricks:
        c = np.array(list(bricks), np.int32).reshape(-1, 3)
        s = np.stack([np.broadcast_to(np.asarray(b[0], F), (8, 8, 8)) for b in bricks.values()])
        w = np.stack([np.broadcast_to(np.asarray(b[1], F), (8, 8, 8)) for b in bricks.values()])
        v.import_bricks(c, s, w)
    return v


FREE = (1.0, 1.0)  # an all-free brick at free_band = VS


def block_answers(ref, corner, conn):
    """The known answers of one free 8^3 block in an unknown field."""
    rel = ref.coords.astype(np.int64) - np.asarray(corner, np.int64)
    k = ((rel == 0) | (rel == 7)).sum(axis=1)
    assert ref.counts["n_voxels"] == 296 and ref.counts["n_free"] == 512
    assert [(k == j).sum() for j in (1, 2, 3)] == [216, 72, 8]
    for j in (1, 2, 3):
        assert set(ref.n_unknown[k == j].tolist()) == {KNOWN[conn][j - 1]}
    if conn == 6:
        assert np.array_equal(ref.dir, (rel == 7).astype(np.int8) - (rel == 0).astype(np.int8))


# ---- 1. the edge of the index domain -------------------------------------------------------------

@pytest.mark.parametrize("b", [0, -1, B20 - 1, -B20])
def test_index_domain_edge(b):
    """One all-free brick at the middle and at the corners of the brick domain: what lies past the
    domain reads unknown.  The brick at -2^20 holds the voxels of index -2^23, which read
    (background, 0) by tsdf_query_dense's |i| < 2^23 rule: its free block is 7^3, as the
    reference says, and the known answers of the 8^3 block hold for the other three."""
    v = volume({(b, b, b): FREE})
    lo, hi = np.full(3, 8 * b - 3, np.int64), np.full(3, 8 * b + 11, np.int64)
    for conn in (6, 18, 26):
        whole = check(v, conn=conn)
        boxed = check(v, lo, hi, conn=conn)
        fr.assert_same((whole.coords, whole.n_unknown, whole.dir), boxed)
        if b != -B20:
            block_answers(whole, [8 * b] * 3, conn)
        else:
            assert whole.counts["n_free"] == 343 and whole.counts["n_voxels"] == 343 - 125
            assert whole.coords.min() == -(1 << 23) + 1
    r = check(v, conn=26, mu=10)
    assert r.counts["n_voxels"] == (80 if b != -B20 else 7 * 12 - 16)
    v.close()


# ---- 2. a neighbour past the key's range must not be packed --------------------------------------

def test_key_aliasing():
    """The +x neighbour of brick (2^20 - 1, 0, 0) has no key; packed unguarded, its x field would
    carry into y and name brick (-2^20, 1, 0), which this map holds fully observed."""
    v = volume({(B20 - 1, 0, 0): FREE, (-B20, 1, 0): (-1.0, 1.0)})
    for conn in (6, 18, 26):
        r = check(v, conn=conn)
        block_answers(r, [8 * (B20 - 1), 0, 0], conn)
        face = r.coords[:, 0] == 8 * B20 - 1
        assert face.sum() == 64 and np.all(r.dir[face, 0] > 0)
    v.close()


# ---- 3. two bricks adjacent across every direction class -----------------------------------------

DIRECTIONS = [d for d in fr.OFFSETS if d > (0, 0, 0)]


@pytest.mark.parametrize("d", DIRECTIONS, ids=lambda d: "%+d%+d%+d" % d)
def test_brick_pairs(d):
    assert len(DIRECTIONS) == 13
    v = volume({(-1, 2, 0): FREE, (-1 + d[0], 2 + d[1], d[2]): FREE})
    shared = {1: 64, 2: 8, 3: 1}[sum(map(abs, d))]
    for conn in (6, 18, 26):
        r = check(v, conn=conn)
        assert r.counts["n_free"] == 1024 and r.counts["n_bricks"] == 2
        if sum(map(abs, d)) == 1:  # a shared face: its 6 x 6 interior voxels are no frontier
            assert r.counts["n_voxels"] == 2 * (296 - 36)
        elif conn == 6:
            assert r.counts["n_voxels"] == 2 * 296
    # the corner voxels that see the other brick at connectivity 26 lose unknown neighbours
    a, b = check(v, conn=26, mu=19), check(v, conn=26, mu=18)
    assert a.counts["n_voxels"] == {64: 8, 8: 12, 1: 14}[shared]
    assert b.counts["n_voxels"] == {64: 8, 8: 12, 1: 16}[shared]
    v.close()


# ---- 4. partly observed neighbours ---------------------------------------------------------------

def test_partly_observed_neighbours():
    z, y, x = np.indices((8, 8, 8))
    board = ((x + y + z) & 1).astype(F)          # W = 0 on a checkerboard
    light = np.where((x + y + z) % 3 == 0, 3.0, 1.0).astype(F)  # W below min_weight = 2 on most
    v = volume({(0, 0, 0): FREE, (1, 0, 0): (1.0, board), (0, 1, 0): (1.0, light),
                (0, 0, 1): (-0.5, 3.0)})
    for conn in (6, 18, 26):
        for mw in (0.0, 2.0):
            r = check(v, conn=conn, mw=mw)
            check(v, [-2, -2, -2], [12, 13, 11], conn=conn, mw=mw, mu=2)
        assert r.counts["n_bricks"] == 4
    lo0, hi0 = check(v, mw=0.0), check(v, mw=2.0)
    assert lo0.counts["n_free"] == 512 + 256 + 512 and hi0.counts["n_free"] == int((light >= 2).sum())
    v.close()


# ---- 5. a seeded random field --------------------------------------------------------------------

def random_bricks(seed, missing=0.33):
    rng = np.random.default_rng(seed)
    out = {}
    for bz in range(3):
        for by in range(3):
            for bx in range(3):
                if rng.random() < missing:
                    continue
                s = rng.uniform(-TAU, TAU, (8, 8, 8)).astype(F)
                w = rng.choice(np.array([0, 1, 3], F), (8, 8, 8))
                out[(bx - 2, by + 1, bz - 1)] = (s, w)
    return out


RANDOM_BOXES = [None, ((-13, 9, -7), (6, 30, 13)), ((-13, 28, 1), (-12, 29, 2)),
                ((-3, 17, 2), (-3, 30, 9)), ((100, 100, 100), (130, 120, 110))]


@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_random_field(sem):
    """Both semantics: the background is tau in one and 0 in the other, and is never observed."""
    bricks = random_bricks(11)
    assert 12 <= len(bricks) <= 24
    v = volume(bricks, semantics=sem)
    S, W = v.query_dense([-17, 7, -9], [-16, 8, -8])
    assert W[0, 0, 0] == 0 and S[0, 0, 0] == F(TAU if sem == "vdbfusion_f64" else 0.0)
    total = 0
    for box in RANDOM_BOXES:
        lo, hi = box if box else (None, None)
        for conn in (6, 18, 26):
            for mu in (1, 3, conn):
                for band in (0.0, VS):
                    r = check(v, lo, hi, band=band, conn=conn, mu=mu)
                    total += r.counts["n_voxels"]
        if box == RANDOM_BOXES[2]:  # a single voxel, which is a frontier voxel at (6, 3, 0)
            assert check(v, lo, hi, band=0.0, conn=6, mu=3).coords.tolist() == [list(lo)]
        if box == RANDOM_BOXES[3] or box == RANDOM_BOXES[4]:  # an empty box, a box off the map
            assert r.counts == ZERO
    check(v, mw=2.0, conn=18, mu=2)
    assert total > 10000
    v.close()


# ---- 6. more listed bricks than the grid cap -----------------------------------------------------

def test_past_the_grid_cap():
    """A flat sheet of GRID_CAP + 3 bricks, one free voxel each at a place that moves with the
    brick: the workgroups stride, against the sparse reference."""
    from tsdf_map import HipTSDFVolume
    n = GRID_CAP + 3
    side = 46
    assert side * side >= n > (side - 1) ** 2
    i = np.arange(n)
    c = np.stack([i % side - 20, i // side + 3, np.full(n, -2)], axis=1).astype(np.int32)
    w = np.zeros((n, 512), F)
    w[i, (i * 37) % 512] = 1.0
    w[i[::5], (i[::5] * 37 + 1) % 512] = 1.0
    s = np.full((n, 512), 1.0, F)
    v = HipTSDFVolume(VS, TAU, **SMALL)
    v.import_bricks(c, s, w)
    r = check(v, conn=26)
    assert r.counts["n_bricks"] == n > GRID_CAP and r.counts["n_frontier_bricks"] == n
    assert r.counts["n_free"] == n + len(i[::5])
    # the last bricks of the list are those of the stride's second trip
    assert np.array_equal(r.coords[-1] >> 3, c[-1])
    check(v, [-100, 0, -16], [8 * 12 + 3, 8 * 40, -9], conn=6)
    v.close()


# ---- 7. the capacity protocol --------------------------------------------------------------------

def test_capacity_protocol():
    from tsdf_map import _abi
    v = volume(random_bricks(12))
    ref = fr.of_bricks(v, VS)
    ref.counts["n_bricks"] = v.num_bricks()
    n = ref.counts["n_voxels"]
    assert n > 100
    for name in NAMES[1:]:
        rc, st, out = raw(v, name, cap=n - 1)
        assert rc == _abi.TSDF_EOVERFLOW and st == ref.counts
        assert all(np.all(a.view(np.uint8) == 0x5A) for a in out)
        rc, st, out = raw(v, name, cap=0, use=(0, 0, 0))
        assert rc == _abi.TSDF_EOVERFLOW and st == ref.counts
        rc, st, out = raw(v, name, cap=n)
        assert rc == _abi.TSDF_OK and st == ref.counts
        fr.assert_same(out, ref)
    rc, st, _ = raw(v, NAMES[0])
    assert rc == _abi.TSDF_OK and st == ref.counts
    v.close()


# ---- 8. determinism: the pool's order does not matter --------------------------------------------

def test_pool_order():
    from tsdf_map import HipTSDFVolume
    bricks = random_bricks(13)
    c = np.array(list(bricks), np.int32)
    s = np.stack([b[0] for b in bricks.values()])
    w = np.stack([b[1] for b in bricks.values()])
    got = []
    for seed in (1, 2):
        p = np.random.default_rng(seed).permutation(c.shape[0])
        h = HipTSDFVolume(VS, TAU, **SMALL)
        half = p.shape[0] // 2
        h.import_bricks(c[p[:half]], s[p[:half]], w[p[:half]])
        h.import_bricks(c[p[half:]], s[p[half:]], w[p[half:]])
        assert not np.array_equal(h.brick_coords(), c[p])  # (the pool holds them in import order)
        f = h.frontiers(connectivity=26)
        got.append(f.coords.tobytes() + f.n_unknown.tobytes() + f.dir.tobytes())
        again = h.frontiers(connectivity=26)
        assert got[-1] == again.coords.tobytes() + again.n_unknown.tobytes() + again.dir.tobytes()
        h.close()
    assert got[0] == got[1] and len(got[0]) > 19 * 100


# ---- 9. the map is left as it was ----------------------------------------------------------------

def test_map_unchanged():
    v = volume(random_bricks(14))
    before = v.export_bricks()
    check(v, conn=18)
    check(v, [-13, 9, -7], [6, 30, 13], conn=26, mu=2)
    after = v.export_bricks()
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    v.close()


# ---- 10 and 11. an integrated map, and the map after it changes ----------------------------------

@pytest.fixture(scope="module")
def carved(scan0):
    from tsdf_map import HipTSDFVolume
    pts, org = scan0
    out = {}
    for sem in ("vdbfusion_f64", "voxblox"):
        v = HipTSDFVolume(VS, TAU, space_carving=True, max_range=40.0, semantics=sem,
                          max_bricks=1 << 16)
        v.integrate(np.ascontiguousarray(pts[::4]), org)
        v.sync()
        out[sem] = v
    yield out
    for v in out.values():
        v.close()


@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_integrated_map(carved, sem):
    """scan0 (every 4th point) integrated with space carving, in the box SCAN_LO .. SCAN_HI."""
    v = carved[sem]
    assert v.space_carving
    n = np.array(SCAN_HI) - np.array(SCAN_LO)
    assert np.all(n <= 96) and np.any(np.array(SCAN_LO) % 8 != 0)
    ref = fr.of_volume(v, SCAN_LO, SCAN_HI, VS)
    seen = np.bincount(ref.n_unknown, minlength=4)
    print("%s box %s..%s: %s, n_unknown histogram %s" % (sem, SCAN_LO, SCAN_HI, ref.counts,
                                                        seen.tolist()))
    assert ref.counts["n_voxels"] >= 1000 and np.all(seen[1:4] > 0)
    check(v, SCAN_LO, SCAN_HI, ref=ref)
    check(v, SCAN_LO, SCAN_HI, conn=26, mu=4, mw=0.5)


def test_changing_maps(carved, sim):
    """After a second integrate, after prune and after evict_outside the result follows the map."""
    v = carved["vdbfusion_f64"]  # (the last test of the module that uses it)
    first = v.frontiers(SCAN_LO, SCAN_HI)
    pts, org = sim.scan(1)
    v.integrate(np.ascontiguousarray(pts[::4]), org)
    v.sync()
    second = check(v, SCAN_LO, SCAN_HI)
    assert second.counts["n_free"] > first.counts["n_free"]
    v.prune(1.5)
    third = check(v, SCAN_LO, SCAN_HI)
    assert third.counts["n_free"] < second.counts["n_free"]
    keep_lo, keep_hi = np.array([1, -3, -2]), np.array([9, 4, 3])  # bricks
    assert v.evict_outside(keep_lo, keep_hi, copy_out=False) > 0
    fourth = check(v, SCAN_LO, SCAN_HI)
    assert 0 < fourth.counts["n_bricks"] < third.counts["n_bricks"]
    whole = check(v)
    assert whole.counts["n_bricks"] == v.num_bricks()
    assert np.all((whole.coords >> 3 >= keep_lo) & (whole.coords >> 3 < keep_hi))


# ---- 12. the entry rules -------------------------------------------------------------------------

def test_entry_rules():
    import torch
    from tsdf_map import HipTSDFVolume, _abi
    v = volume(random_bricks(15))
    nan, inf = float("nan"), float("inf")
    box = dict(lo=[-13, 9, -7], hi=[6, 30, 13])
    n = v.frontier_counts(**box)["n_voxels"]
    assert n > 0

    def refused(message, names=NAMES, **kw):
        for name in names:
            rc, st, out = raw(v, name, cap=n, **{**box, **kw})
            assert rc == _abi.TSDF_EINVAL and text(v) == "frontier: " + message, (name, text(v))
            assert out is None or all(np.all(a.view(np.uint8) == 0x5A) for a in out
                                      if a is not None)

    # each rule alone, then with every later rule broken as well: the first one is reported
    later = [dict(hi=None), dict(band=nan), dict(mw=-1.0), dict(conn=7), dict(mu=0),
             dict(hi=[6, 8, 13]), dict(lo=[-(1 << 31), 9, -7])]
    texts = ["lo and hi must both be given or both be NULL", "free_band is not finite",
             "min_weight is negative or NaN", "connectivity must be 6, 18 or 26",
             "min_unknown must be in 1..connectivity", "hi < lo", "box extent >= 2^31 voxels"]
    for k, (kw, message) in enumerate(zip(later, texts)):
        refused(message, **kw)
        merged = {}
        for other in reversed(later[k:]):
            merged.update(other)
        if k == 0:
            merged["hi"] = None
        if k < 5:  # (the two box rules share lo / hi: ORDER is reported before EXTENT)
            refused(message, **merged)
    refused("lo and hi must both be given or both be NULL", lo=None)
    refused("free_band is not finite", band=inf)
    refused("min_weight is negative or NaN", mw=nan)
    for conn, mu in ((6, 7), (18, 19), (26, 27), (26, -1)):
        refused("min_unknown must be in 1..connectivity", conn=conn, mu=mu)
    refused("hi < lo", lo=[0, 0, 0], hi=[1 << 40, -1, 0])
    refused("box extent >= 2^31 voxels", lo=[-(1 << 62), 0, 0], hi=[1 << 62, 8, 8])
    # a NULL out
    for name in NAMES:
        fn = getattr(v._lib, name)
        args = (v._ctx, None, None, VS, 0.0, 6, 1)
        rc = fn(*args, None) if name == NAMES[0] else fn(*args, None, None, None, 0, None)
        assert rc == _abi.TSDF_EINVAL and text(v) == "frontier: null counts"
    # a NULL coords where there are frontier voxels and cap suffices; too small a cap comes first
    refused("null buffer", names=NAMES[1:], use=(0, 1, 1))
    for name in NAMES[1:]:
        rc, st, _ = raw(v, name, cap=n - 1, use=(0, 1, 1), **box)
        assert rc == _abi.TSDF_EOVERFLOW and st["n_voxels"] == n
    # an empty box and a box that misses every brick return zeros; so does an empty map
    e = HipTSDFVolume(VS, TAU, **SMALL)
    for name in NAMES:
        for vol, kw in ((v, dict(lo=[0, 0, 0], hi=[8, 0, 8])),
                        (v, dict(lo=[1 << 40, 0, 0], hi=[(1 << 40) + 5, 8, 8])),
                        (v, dict(lo=[800, 800, 800], hi=[900, 900, 900])), (e, {}), (e, box)):
            rc, st, out = raw(vol, name, cap=4, use=(0, 0, 0), **kw)
            assert rc == _abi.TSDF_OK and st == ZERO, (name, kw, text(vol))
    s = e.frontiers()
    assert len(s) == 0 and s.coords.shape == (0, 3) and s.clusters() == []
    assert [tuple(t.shape) for t in e.frontiers_device()[:3]] == [(0, 3), (0,), (0, 3)]
    e.close()
    # the Python layer's own rules
    for kw in (dict(connectivity=7), dict(min_unknown=0), dict(connectivity=6, min_unknown=7)):
        with pytest.raises(ValueError):
            v.frontiers(**kw)
    with pytest.raises(ValueError):
        v.frontiers(lo=[0, 0, 0])
    # one sector shard of two
    sh = HipTSDFVolume(VS, TAU, n_sectors=2, sector=0, **SMALL)
    for name in NAMES:
        rc, _, _ = raw(sh, name)
        assert rc == _abi.TSDF_EINVAL and "n_sectors > 1" in text(sh)
        assert text(sh).startswith("frontier: ")
    sh.close()
    # an open border reduce
    a, b = (volume({(0, 0, 0): FREE, (1, 0, 0): FREE}) for _ in range(2))
    nb = a.num_bricks()
    dev = torch.device("cuda", 0)
    allk = torch.full((2, nb), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for r, vol in enumerate((a, b)):
        assert vol.brick_keys_into(allk[r].data_ptr(), nb) == nb
    send = torch.empty((nb, 1028), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    counts, sent = np.array([nb, nb], np.uint64), np.zeros(2, np.uint64)
    rc = b._lib.tsdf_border_pack_device(b._ctx, C.c_void_p(allk.data_ptr()),
                                        counts.ctypes.data_as(_abi.U64P), nb, 2, 1,
                                        C.c_void_p(send.data_ptr()), nb,
                                        sent.ctypes.data_as(_abi.U64P))
    assert rc == _abi.TSDF_OK and sent.tolist() == [nb, 0], text(b)
    for name in NAMES:
        rc, _, _ = raw(b, name)
        assert rc == _abi.TSDF_EINVAL and text(b).startswith("frontier: a border reduce is open")
    b.border_commit(False)
    rc, st, _ = raw(b, NAMES[0])
    assert rc == _abi.TSDF_OK and st == a.frontier_counts(), text(b)
    a.close()
    b.close()
    v.close()


def test_frontiers_around_and_clusters(carved):
    from tsdf_map import frontiers_around
    from tsdf_map.esdf import box_around
    v = carved["voxblox"]
    centre, half = [5.0, 0.0, 0.5], [2.0, 2.0, 1.0]
    s = frontiers_around(v, centre, half, connectivity=18)
    lo, hi = box_around(centre, half, v.voxel_size)
    ref = fr.of_volume(v, lo, hi, VS, 0.0, 18, 1)
    fr.assert_same((s.coords, s.n_unknown, s.dir), ref)
    cl = s.clusters(min_voxels=5)
    assert cl and cl[0].size >= cl[-1].size >= 5
    assert sum(c.size for c in s.clusters()) == len(s)
