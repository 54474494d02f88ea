"""The indexed mesh on the GPU (include/tsdf_hip_mesh.h): vertices, normals and triangles equal
tests/meshref.py bit for bit, and de-indexed they are the GPU's own soup, on a sphere, a field with
holes and low weights, a missing neighbour brick, an integrated scan and boxes that cut bricks; the
capacity protocol, the device outputs, the refusals, and independence of the pool's order; and a
sphere of more bricks than the per-brick kernels' grid cap (tests/pastcap.py)."""
import ctypes as C

import numpy as np
import pytest

import meshref
import pastcap as pc
from test_mesh import TAU, VS, sphere_bricks
from tsdf_map import HipTSDFVolume, _abi, load_hip_library
from tsdf_map.mesh import mesh_tiles, tile_boxes

pytestmark = pytest.mark.gpu

SMALL = dict(max_bricks=1 << 12, max_points=1 << 13, max_batch=4)
# the surface crosses the brick faces at voxel 0 on every axis, at -8 on y and at +8 on x and z
CENTER = (0.113, -0.121, 0.207)
TABLES = ["generated", "lorensen"]
VOXBLOX_MIN_WEIGHT = 1.5  # between one observation (W <= 1) and two


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def table(name):
    return meshref.mc_table(load_hip_library(), _abi.MC_TABLES[name])


def volume(bricks, **kw):
    g = HipTSDFVolume(VS, TAU, **dict(SMALL, **kw))
    g.import_bricks(*bricks)
    return g


def same_mesh(got, ref):
    """got: (vertices, triangles, normals) of the volume; ref: (vertices, normals, triangles)."""
    v, t, n = got
    rv, rn, rt = ref
    assert v.dtype == np.float32 and t.dtype == np.uint32 and n.dtype == np.float32
    assert v.shape == rv.shape and t.shape == rt.shape and n.shape == rn.shape
    assert np.array_equal(t, rt)
    assert np.array_equal(u32(v), u32(rv))
    assert np.array_equal(u32(n), u32(rn))


def check_whole(g, dense, tname, min_weight=0.0, least=50):
    got = g.extract_indexed_mesh(min_weight=min_weight, table=tname)
    ref = meshref.indexed_mesh_ref(*dense, VS, table(tname), min_weight=min_weight)
    assert ref[2].shape[0] > least
    same_mesh(got, ref)
    soup, _ = g.extract_triangle_mesh(min_weight=min_weight, table=tname)
    assert np.array_equal(u32(meshref.deindex(got[0], got[1])), u32(soup))
    return got


@pytest.fixture(scope="module")
def sphere():
    """(bricks, dense, volume) of the offset sphere; the tests that use it only read."""
    b = sphere_bricks(0.37, center=CENTER)
    g = volume(b)
    yield b, meshref.dense_from_bricks(*b), g
    g.close()


@pytest.fixture(scope="module")
def holed():
    """The sphere with a seeded 10 % of the voxels unobserved and 5 % at W = 0.5."""
    c, s, w = sphere_bricks(0.37, center=CENTER)
    w = meshref.holed(w)
    low = np.random.default_rng(3).random(w.shape) < 0.05
    w = np.where(low & (w > 0), np.float32(0.5), w).astype(np.float32)
    g = volume((c, s, w))
    yield (c, s, w), meshref.dense_from_bricks(c, s, w), g
    g.close()


@pytest.mark.parametrize("tname", TABLES)
def test_sphere_parity(sphere, tname):
    _, dense, g = sphere
    v, t, n = check_whole(g, dense, tname)
    assert np.unique(t).shape[0] == v.shape[0] and v.shape[0] * 2 - 4 == t.shape[0]  # closed
    # without normals: the same vertices and triangles
    v2, t2, n2 = g.extract_indexed_mesh(table=tname, normals=False)
    assert n2 is None and np.array_equal(u32(v2), u32(v)) and np.array_equal(t2, t)


@pytest.mark.parametrize("tname,min_weight", [("generated", 0.0), ("lorensen", 0.0),
                                              ("generated", 0.75), ("lorensen", 1.0)])
def test_holes_and_min_weight(holed, tname, min_weight):
    """Edges with 1 to 3 meshed cubes, and vertices owned by bricks whose own cubes emit nothing."""
    _, dense, g = holed
    v, t, n = check_whole(g, dense, tname, min_weight)
    info = {}
    meshref.indexed_mesh_ref(*dense, VS, table(tname), min_weight=min_weight, info=info)
    assert {1, 2, 3} <= set(info["cubes_per_vertex"].tolist())
    if min_weight:
        full = g.indexed_mesh_counts(table=tname)
        assert 0 < t.shape[0] < full["n_triangles"]


def test_missing_neighbour_brick(sphere):
    """The bricks at x <= 0 only: the surface runs into faces whose +x neighbour is absent."""
    (c, s, w), _, _ = sphere
    keep = c[:, 0] <= 0
    b = (c[keep], s[keep], w[keep])
    g = volume(b)
    v, t, n = check_whole(g, meshref.dense_from_bricks(*b), "generated")
    full = sphere[2].indexed_mesh_counts()
    assert t.shape[0] < full["n_triangles"]
    g.close()


def integrated_scan(sim, semantics, min_weights, **kw):
    """A few thousand rays of one generated scan: the reference from query_dense of the touched
    box."""
    pts, org = sim.scan(0)
    vs = 0.1
    g = HipTSDFVolume(vs, 3 * vs, semantics=semantics, **dict(SMALL, **kw))
    g.integrate(np.ascontiguousarray(pts[20000:20000 + 6144]), org)
    c = g.brick_coords()
    assert 50 < c.shape[0] < 1000
    lo, hi = c.min(0).astype(np.int64) * 8 - 2, (c.max(0).astype(np.int64) + 1) * 8 + 2
    S, W = g.query_dense(lo, hi)
    tab = table("generated")
    for mw in min_weights:
        ref = meshref.indexed_mesh_ref(S, W, lo, vs, tab, min_weight=mw)
        print("%s min_weight %g: %d vertices, %d triangles" % (semantics, mw, ref[0].shape[0],
                                                               ref[2].shape[0]))
        assert ref[2].shape[0] > (1000 if mw == 0.0 else 50)
        got = g.extract_indexed_mesh(min_weight=mw)
        same_mesh(got, ref)
        soup, _ = g.extract_triangle_mesh(min_weight=mw)
        assert np.array_equal(u32(meshref.deindex(got[0], got[1])), u32(soup))
    g.close()
    return W


def test_integrated_scan(sim):
    integrated_scan(sim, "vdbfusion_f64", (0.0, 2.0))


def test_integrated_scan_voxblox(sim):
    """The same in the Voxblox semantics: background 0, and weights that drop off behind the
    surface, so that a min_weight of 1.5 removes about three quarters of the observed voxels."""
    W = integrated_scan(sim, "voxblox", (0.0, VOXBLOX_MIN_WEIGHT), max_range=40.0)
    seen = W[W > 0]
    assert (seen < VOXBLOX_MIN_WEIGHT).sum() >= 1000 and (seen >= VOXBLOX_MIN_WEIGHT).sum() >= 1000


def test_box_partition(sphere):
    """Boxes of 13 voxels cut the bricks at planes that are no multiples of 8: every piece equals
    the reference with that box, the pieces' triangles together are the soup, and mesh_tiles
    yields the same pieces."""
    (c, _, _), dense, g = sphere
    tab = table("generated")
    boxes = tile_boxes(c, 13)
    assert len(boxes) > 27 and all(np.any(lo % 8 != 0) or np.any(hi % 8 != 0) for lo, hi in boxes)
    tiles = list(mesh_tiles(g, 13))
    assert len(tiles) == len(boxes)
    rows, filled = [], 0
    for (lo, hi), (tlo, thi, got) in zip(boxes, tiles):
        assert np.array_equal(lo, tlo) and np.array_equal(hi, thi)
        ref = meshref.indexed_mesh_ref(*dense, VS, tab, lo=lo, hi=hi)
        same_mesh(got, ref)
        direct = g.extract_indexed_mesh(lo=lo, hi=hi)
        same_mesh(direct, ref)
        rows.append(u32(meshref.deindex(got[0], got[1])).reshape(-1, 9))
        filled += got[1].shape[0] > 0
    assert filled >= 8
    soup, _ = g.extract_triangle_mesh()
    rows = np.concatenate(rows)
    want = u32(soup).reshape(-1, 9)
    assert rows.shape == want.shape
    order = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
    assert np.array_equal(order(rows), order(want))
    # a box that is one voxel thick, and one inside a single brick
    for lo, hi in (([-30, -30, 3], [30, 30, 4]), ([1, -7, 2], [7, -1, 7])):
        same_mesh(g.extract_indexed_mesh(lo=lo, hi=hi),
                  meshref.indexed_mesh_ref(*dense, VS, tab, lo=lo, hi=hi))


def raw(g, fn_name, min_weight=0.0, tab=0, lo=None, hi=None, v=None, n=None, t=None, cap_v=0,
        cap_t=0, counts=True):
    """A call of the C entry point: (rc, counts dict)."""
    fn = getattr(g._lib, fn_name)
    st = _abi.MeshCounts(7, 7, 7)
    plo = None if lo is None else np.asarray(lo, np.int64).ctypes.data_as(_abi.L3)
    phi = None if hi is None else np.asarray(hi, np.int64).ctypes.data_as(_abi.L3)
    out = C.byref(st) if counts else None
    if fn_name == "tsdf_mesh_indexed_count":
        rc = fn(g._ctx, min_weight, tab, plo, phi, out)
    else:
        rc = fn(g._ctx, min_weight, tab, plo, phi,
                None if v is None else v.ctypes.data_as(_abi.FP),
                None if n is None else n.ctypes.data_as(_abi.FP),
                None if t is None else t.ctypes.data_as(_abi.U32P), cap_v, cap_t, out)
    return rc, st.as_dict()


def text(v):
    return v._lib.tsdf_last_error(v._ctx).decode()


def test_capacities_and_device_outputs(sphere):
    import torch
    _, dense, g = sphere
    before = g.export_bricks()
    ref = meshref.indexed_mesh_ref(*dense, VS, table("generated"))
    nv, nt = ref[0].shape[0], ref[2].shape[0]
    rc, cnt = raw(g, "tsdf_mesh_indexed_count")
    assert rc == _abi.TSDF_OK and cnt == {"n_bricks": g.num_bricks(), "n_vertices": nv,
                                          "n_triangles": nt}
    sentinel = np.float32(-7.5)
    for cap_v, cap_t in ((nv - 1, nt), (nv, nt - 1), (0, 0)):
        v = np.full((nv, 3), sentinel, np.float32)
        n = np.full((nv, 3), sentinel, np.float32)
        t = np.full((nt, 3), 0xABCDEF01, np.uint32)
        rc, got = raw(g, "tsdf_mesh_indexed", v=v, n=n, t=t, cap_v=cap_v, cap_t=cap_t)
        assert rc == _abi.TSDF_EOVERFLOW and got == cnt
        assert text(g) == "mesh has %d vertices and %d triangles" % (nv, nt)
        assert np.all(v == sentinel) and np.all(n == sentinel) and np.all(t == 0xABCDEF01)
    v = np.full((nv + 1, 3), sentinel, np.float32)
    n = np.full((nv + 1, 3), sentinel, np.float32)
    t = np.full((nt + 1, 3), 0xABCDEF01, np.uint32)
    rc, got = raw(g, "tsdf_mesh_indexed", v=v, n=n, t=t, cap_v=nv + 1, cap_t=nt + 1)
    assert rc == _abi.TSDF_OK and got == cnt, text(g)
    same_mesh((v[:nv], t[:nt], n[:nv]), ref)
    assert np.all(v[nv] == sentinel) and np.all(n[nv] == sentinel) and np.all(t[nt] == 0xABCDEF01)
    # the device variant: the same arrays, and the same protocol
    dv, dt, dn = g.indexed_mesh_device()
    assert dv.is_cuda and dt.dtype == torch.uint32
    same_mesh((dv.cpu().numpy(), dt.cpu().numpy(), dn.cpu().numpy()), ref)
    dv2, dt2, dn2 = g.indexed_mesh_device(normals=False, lo=[-30, -30, 3], hi=[30, 30, 9])
    hv, ht, _ = g.extract_indexed_mesh(normals=False, lo=[-30, -30, 3], hi=[30, 30, 9])
    assert dn2 is None and 0 < ht.shape[0] < nt
    assert np.array_equal(u32(dv2.cpu().numpy()), u32(hv)) and np.array_equal(dt2.cpu().numpy(), ht)
    buf = torch.full((nv * 3,), -7.5, dtype=torch.float32, device=g.tensor_device)
    idx = torch.full((nt * 3,), 5, dtype=torch.int32, device=g.tensor_device)
    torch.cuda.synchronize()
    st = _abi.MeshCounts()
    rc = g._lib.tsdf_mesh_indexed_device(g._ctx, 0.0, 0, None, None, C.c_void_p(buf.data_ptr()),
                                         None, C.c_void_p(idx.data_ptr()), nv, nt - 1,
                                         C.byref(st))
    assert rc == _abi.TSDF_EOVERFLOW and st.as_dict() == cnt
    assert bool((buf == -7.5).all()) and bool((idx == 5).all())
    # the map is as it was
    after = g.export_bricks()
    assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(before, after))


def test_refusals(sphere):
    import torch
    _, _, g = sphere
    nan = float("nan")
    good = dict(lo=[0, 0, 0], hi=[8, 8, 8])
    for name in ("tsdf_mesh_indexed_count", "tsdf_mesh_indexed", "tsdf_mesh_indexed_device"):
        def refused(msg=None, **kw):
            rc, st = raw(g, name, **kw)
            assert rc == _abi.TSDF_EINVAL and text(g), (name, kw, rc, text(g))
            if msg:
                assert msg in text(g), text(g)
            assert st == {"n_bricks": 7, "n_vertices": 7, "n_triangles": 7}
        refused("null counts", counts=False)
        refused("table", tab=-1)
        refused("table", tab=3)
        refused("min_weight", min_weight=-1.0)
        refused("min_weight", min_weight=nan)
        refused("both", lo=[0, 0, 0])
        refused("both", hi=[8, 8, 8])
        refused("hi < lo", lo=[0, 0, 0], hi=[8, -1, 8])
        refused("2^31", lo=[0, -(1 << 30), 0], hi=[8, 1 << 30, 8])
        refused("2^31", lo=[-(1 << 62), 0, 0], hi=[1 << 62, 8, 8])
        # an empty box returns zeros
        rc, st = raw(g, name, lo=[0, 0, 0], hi=[8, 0, 8])
        assert rc == _abi.TSDF_OK and st == {"n_bricks": 0, "n_vertices": 0, "n_triangles": 0}
        rc, st = raw(g, name, lo=[1 << 40, 0, 0], hi=[(1 << 40) + 5, 8, 8])  # no brick there
        assert rc == _abi.TSDF_OK and st == {"n_bricks": 0, "n_vertices": 0, "n_triangles": 0}
    # NULL outputs where the mesh is not empty and the capacities would do
    rc, _ = raw(g, "tsdf_mesh_indexed", cap_v=1 << 20, cap_t=1 << 20, **good)
    assert rc == _abi.TSDF_EINVAL and text(g) == "mesh: null buffer"
    # an empty map
    e = HipTSDFVolume(VS, TAU, **SMALL)
    for name in ("tsdf_mesh_indexed_count", "tsdf_mesh_indexed", "tsdf_mesh_indexed_device"):
        rc, st = raw(e, name)
        assert rc == _abi.TSDF_OK and st == {"n_bricks": 0, "n_vertices": 0, "n_triangles": 0}
    assert [a.shape for a in e.extract_indexed_mesh()] == [(0, 3)] * 3
    e.close()
    # one sector shard of two
    s = HipTSDFVolume(VS, TAU, n_sectors=2, sector=0, **SMALL)
    rc, _ = raw(s, "tsdf_mesh_indexed_count")
    assert rc == _abi.TSDF_EINVAL and "n_sectors > 1" in text(s)
    s.close()
    # an open border reduce
    a, b = (volume(sphere[0]) for _ in range(2))
    nb = a.num_bricks()
    dev = torch.device("cuda", 0)
    allk = torch.full((2, nb), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for r, v in enumerate((a, b)):
        assert v.brick_keys_into(allk[r].data_ptr(), nb) == nb
    send = torch.empty((nb, 1028), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    counts, sent = np.array([nb, nb], np.uint64), np.zeros(2, np.uint64)
    rc = b._lib.tsdf_border_pack_device(b._ctx, C.c_void_p(allk.data_ptr()),
                                        counts.ctypes.data_as(_abi.U64P), nb, 2, 1,
                                        C.c_void_p(send.data_ptr()), nb,
                                        sent.ctypes.data_as(_abi.U64P))
    assert rc == _abi.TSDF_OK and sent.tolist() == [nb, 0], text(b)
    for name in ("tsdf_mesh_indexed_count", "tsdf_mesh_indexed", "tsdf_mesh_indexed_device"):
        rc, _ = raw(b, name)
        assert rc == _abi.TSDF_EINVAL and "a border reduce is open" in text(b)
    b.border_commit(False)
    rc, st = raw(b, "tsdf_mesh_indexed_count")
    assert rc == _abi.TSDF_OK and st == a.indexed_mesh_counts(), text(b)
    a.close()
    b.close()


def test_pool_order(holed):
    """The same bricks imported in two shuffled orders (two pool orders): identical output."""
    (c, s, w), dense, g = holed
    want = g.extract_indexed_mesh(min_weight=0.75)
    for seed in (1, 2):
        p = np.random.default_rng(seed).permutation(c.shape[0])
        h = HipTSDFVolume(VS, TAU, **SMALL)
        half = p.shape[0] // 2
        h.import_bricks(c[p[:half]], s[p[:half]], w[p[:half]])
        h.import_bricks(c[p[half:]], s[p[half:]], w[p[half:]])
        got = h.extract_indexed_mesh(min_weight=0.75)
        same_mesh(got, (want[0], want[2], want[1]))
        h.close()


# ---- more bricks than the grid cap ---------------------------------------------------------------

LARGE = dict(max_bricks=1 << 13)


@pytest.fixture(scope="module")
def large():
    """kind -> volume of the 18^3-brick sphere (tests/pastcap.py); the tests only read."""
    out = {kind: volume(pc.mesh_map(kind), **LARGE) for kind in ("full", "holed")}
    yield out
    for g in out.values():
        g.close()


def check_large(g, kind, tname, min_weight, boxed):
    """The volume's mesh against pastcap's reference of the same case, whose conditions are
    asserted again; returns the volume's mesh."""
    assert np.array_equal(table(tname), pc.mc_table(tname))
    ref, sides = pc.mesh_case(kind, tname, min_weight, boxed)
    print("%s %s min_weight %g %s: %s" % (kind, tname, min_weight, "box" if boxed else "whole",
                                          sides))
    pc.assert_mesh_past_cap(sides)
    lo, hi = pc.MESH_BOX if boxed else (None, None)
    got = g.extract_indexed_mesh(min_weight=min_weight, table=tname, lo=lo, hi=hi)
    same_mesh(got, ref)
    # (n_bricks counts the bricks that hold a voxel of the box; the kernels also list the owners
    # of the vertices on its high faces, which sides["n_bricks"] counts)
    examined = pc.mesh_listed(pc.mesh_map(kind)[0], lo, hi - 1).shape[0] if boxed else \
        sides["n_bricks"]
    cnt = g.indexed_mesh_counts(min_weight=min_weight, table=tname, lo=lo, hi=hi)
    assert cnt == {"n_bricks": examined, "n_vertices": sides["n_vertices"],
                   "n_triangles": sides["n_triangles"]}
    return got


@pytest.mark.parametrize("kind,tname,min_weight", [("full", "generated", 0.0),
                                                   ("holed", "lorensen", 0.75)])
def test_past_the_grid_cap(large, kind, tname, min_weight):
    """5832 bricks against the cap of 4096 workgroups: the bricks from (1, 2, 3) on are meshed on
    a workgroup's second trip, and the triangles around z = 24 index vertices of both trips."""
    g = large[kind]
    v, t, n = check_large(g, kind, tname, min_weight, False)
    soup, _ = g.extract_triangle_mesh(min_weight=min_weight, table=tname)
    assert np.array_equal(u32(meshref.deindex(v, t)), u32(soup))
    if kind == "full":
        assert np.unique(t).shape[0] == v.shape[0] and v.shape[0] * 2 - 4 == t.shape[0]  # closed


def test_box_past_the_grid_cap(large):
    """A box that cuts bricks and lists 4860 of them, more than the cap."""
    g = large["full"]
    v, t, n = check_large(g, "full", "generated", 0.0, True)
    assert 0 < t.shape[0] < g.indexed_mesh_counts()["n_triangles"]


def test_device_outputs_past_the_grid_cap(large):
    g = large["full"]
    ref, sides = pc.mesh_case("full", "generated", 0.0, False)
    pc.assert_mesh_past_cap(sides)
    dv, dt, dn = g.indexed_mesh_device()
    same_mesh((dv.cpu().numpy(), dt.cpu().numpy(), dn.cpu().numpy()), ref)
    hv, ht, hn = g.extract_indexed_mesh()
    same_mesh((dv.cpu().numpy(), dt.cpu().numpy(), dn.cpu().numpy()), (hv, hn, ht))


def test_pool_order_past_the_grid_cap():
    """The bricks imported in reverse order behind a decoy that is then evicted: every brick's
    pool slot differs from its position in the sorted list, before the cap and past it."""
    c, s, w = pc.mesh_map("full")
    assert np.array_equal(c, pc.mesh_listed(c))  # (z, y, x) order: position = row
    h = HipTSDFVolume(VS, TAU, **dict(SMALL, **LARGE))
    h.import_bricks(np.array([[500, 500, 500]], np.int32), s[:1], w[:1])
    h.import_bricks(c[::-1], s[::-1], w[::-1])
    assert h.evict_outside((-400, -400, -400), (400, 400, 400), copy_out=False) == 1
    assert h.num_bricks() == c.shape[0] > pc.MESH_CAP
    check_large(h, "full", "generated", 0.0, False)
    h.close()


def test_vertex_counts_past_their_grid_cap():
    """k_mesh_vcount takes four bricks a workgroup, so its second trip starts at brick 16 384: a
    sphere of 26^3 bricks.  No numpy reference at this size; a wrong count moves every later
    brick's first vertex, so the de-indexed mesh is held to the GPU's own soup, and the surface
    is closed."""
    sides = pc.mesh_big_sides()
    print("26^3 bricks: %s" % sides)
    pc.assert_mesh_vcount_past_cap(sides)
    g = volume(pc.mesh_big_map(), max_bricks=1 << 15)
    v, t, n = g.extract_indexed_mesh()
    soup, _ = g.extract_triangle_mesh()
    assert t.shape[0] * 3 == soup.shape[0] > 0
    assert np.array_equal(u32(meshref.deindex(v, t)), u32(soup))
    assert int(t.max()) + 1 == v.shape[0] == np.unique(t).shape[0]
    assert v.shape[0] * 2 - 4 == t.shape[0]  # closed
    nn = np.linalg.norm(n.astype(np.float64), axis=1)
    assert np.all((np.abs(nn - 1) < 1e-6) | (nn == 0)) and (nn > 0).mean() > 0.99
    assert g.indexed_mesh_counts() == {"n_bricks": sides["n_bricks"], "n_vertices": v.shape[0],
                                       "n_triangles": t.shape[0]}
    # the vertices of the last bricks, which the later trips counted, lie on the sphere's top
    top = v[v[:, 2] >= np.float32(88.5) * np.float32(VS)]
    assert top.shape[0] >= sides["vertices_past"]
    r = np.linalg.norm(top.astype(np.float64) - np.array(pc.MESH_BIG_CENTER), axis=1)
    assert np.all(np.abs(r - pc.MESH_BIG_RADIUS) < VS)
    g.close()
