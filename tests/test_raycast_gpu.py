"""The raycast on the GPU (include/tsdf_hip_raycast.h) against tests/rayref.py, bit for bit: the
reference marches the full lattice on the GPU context's own export_voxels(), which is bitwise the
oracle's, so what test_raycast_ref.py pins on the CPU is what the kernel -- with its brick skip,
its slot cache and its early exit -- is held to here."""
import ctypes as C

import numpy as np
import pytest

import pastcap as pc
import rayref as rr
import sampleref as sr

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"nearest": rr.NEAREST, "trilinear": rr.TRILINEAR}
VS, TAU = sr.VOXEL_SIZE, sr.SDF_TRUNC


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same(got, ref):
    """(depth, normal, hit) of the library against the reference's, bitwise."""
    gd, gn, gh = got
    rd, rn, rh = ref
    assert np.array_equal(np.asarray(gh).astype(np.uint8), rh)
    assert np.array_equal(bits(gd), bits(rd))
    if gn is not None:
        assert np.array_equal(bits(gn), bits(rn))


class Map:
    def __init__(self, vol, rays):
        self.vol = vol
        self.field = sr.field_of(vol)
        self.rays = rays  # name -> (origin (3,) or (n, 3), dirs (n, 3))
        self.ref = {}

    def reference(self, name, mode, mw, step):
        """The reference's raycast of a shared ray set, computed once per case."""
        k = (name, mode, mw, step)
        if k not in self.ref:
            o, d = self.rays[name]
            self.ref[k] = rr.raycast(self.field, o, d, None, rr.T_MIN, rr.T_MAX, step, MODES[mode],
                                     mw)
        return self.ref[k]


@pytest.fixture(scope="module")
def scans(sim):
    return [sim.scan(k) for k in range(rr.N_SCANS)]


@pytest.fixture(scope="module")
def scan_rays(scans):
    return rr.scan_rays(*scans[0])


@pytest.fixture(scope="module")
def maps(scans, scan_rays):
    from tsdf_map import HipTSDFVolume
    org, dirs, _ = scan_rays
    assert dirs.shape == (2048, 3)
    rays = {"scan": (org, dirs), "displaced": ((org + np.array(rr.DISPLACED, F)).astype(F), dirs),
            "reversed": (org, np.ascontiguousarray(-dirs))}
    out = {}
    for sem in ("vdbfusion_f64", "voxblox"):
        v = HipTSDFVolume(VS, TAU, semantics=sem)
        for pts, o in scans:
            v.integrate(pts, o)
        v.sync()
        out[sem] = Map(v, rays)
    assert out["voxblox"].field.bg == 0 and out["vdbfusion_f64"].field.bg == F(TAU)
    yield out
    for m in out.values():
        m.vol.close()


@pytest.mark.parametrize("step", [0.1, 0.05, 0.03])
@pytest.mark.parametrize("min_weight", [0.0, 2.0])
@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
@pytest.mark.parametrize("rayset", ["scan", "displaced"])
@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_raycast_bitwise(maps, sem, rayset, mode, min_weight, step):
    m = maps[sem]
    o, d = m.rays[rayset]
    o = np.broadcast_to(o, d.shape)
    ref = m.reference(rayset, mode, min_weight, step)
    if step == 0.05 and (sem, rayset, min_weight) in rr.HITS:
        assert int(ref[2].sum()) == rr.HITS[(sem, rayset, min_weight)][MODES[mode]]
    if (ref[2] == 0).sum() < 100:  # every ray hits: the same rays turned round are known misses
        back = m.reference("reversed", mode, min_weight, step)
        o, d = np.concatenate([o, o]), np.concatenate([d, m.rays["reversed"][1]])
        ref = tuple(np.concatenate([a, b]) for a, b in zip(ref, back))
    hits, misses = int(ref[2].sum()), int((ref[2] == 0).sum())
    print("%s %s %s min_weight %g step %g: %d hits, %d misses" % (sem, rayset, mode, min_weight,
                                                                  step, hits, misses))
    assert hits >= 100 and misses >= 100
    got = m.vol.raycast(o, d, None, rr.T_MIN, rr.T_MAX, step, mode, min_weight)
    assert_same(got, ref)
    # unit normals, or none where the cube around the hit point is not observed (nearest: often)
    nn = np.linalg.norm(got[1][got[2]].astype(np.float64), axis=1)
    assert np.all((np.abs(nn - 1) < 1e-6) | (nn == 0))
    assert (nn > 0).mean() > (0.99 if mode == "trilinear" else 0.2)


def test_pose(maps, scan_rays):
    """Sensor-frame rays under a pose equal the reference's transform-then-march, and the
    pre-transformed rays with pose = NULL give the same bits."""
    m = maps["vdbfusion_f64"]
    org, dirs, _ = scan_rays
    T = np.eye(4)
    T[:3, :3] = sr.exp_so3([0.02, -0.03, 0.7])
    T[:3, 3] = org.astype(np.float64) + [0.05, 0.02, -0.01]
    d_s = np.ascontiguousarray((dirs[::4].astype(np.float64) @ T[:3, :3]).astype(F))  # R^T d
    o_s = np.zeros_like(d_s)
    o_s[1::2] = [0.01, -0.02, 0.03]  # a beam offset in the sensor frame
    for mode in MODES:
        ref = rr.raycast(m.field, o_s, d_s, T[:3], rr.T_MIN, rr.T_MAX, rr.STEP, MODES[mode])
        assert 50 <= ref[2].sum()
        got = m.vol.raycast(o_s, d_s, T, rr.T_MIN, rr.T_MAX, rr.STEP, mode)
        assert_same(got, ref)
        assert_same(m.vol.raycast(o_s, d_s, T[:3], rr.T_MIN, rr.T_MAX, rr.STEP, mode), ref)
        o_w, d_w = rr.rays_of(o_s, d_s, T[:3])
        assert not np.array_equal(d_w, d_s)
        assert_same(m.vol.raycast(o_w, d_w, None, rr.T_MIN, rr.T_MAX, rr.STEP, mode), ref)


def edge_rays(field, voxels, scan_rays):
    """Named groups of (origins, directions) for one call with t in [0, 3]."""
    org, dirs, rng = scan_rays
    org64, d64 = org.astype(np.float64), dirs.astype(np.float64)
    vs = float(field.vs)
    g = {}
    # NaN and +-inf in each origin and direction component, on a ray that otherwise hits
    base_o = org64 + (rng[0] - 1.5) * d64[0]
    bad_o, bad_d = [], []
    for a in range(3):
        for v in (np.nan, np.inf, -np.inf):
            o, d = base_o.copy(), d64[0].copy()
            o[a] = v
            bad_o.append(o)
            bad_d.append(d64[0])
            d[a] = v
            bad_o.append(base_o)
            bad_d.append(d)
    g["nonfinite"] = (np.array(bad_o), np.array(bad_d))
    # 1.5 m in front of the measured surface: hits; the same with a zero direction: none
    sel = slice(0, 2048, 8)
    near = org64 + (rng[sel, None] - 1.5) * d64[sel]
    g["near"] = (near, d64[sel])
    g["zero_dir"] = (near[:32], np.zeros((32, 3)) * np.array([1.0, -1.0, 1.0]))
    # starting behind the surface (S < 0), on rays that end on the outer wall: nothing beyond
    end = org64 + rng[:, None] * d64
    wall = np.hypot(end[:, 0], end[:, 1]) > 24.5
    g["behind"] = ((org64 + (rng[:, None] + 0.15) * d64)[wall][:256], d64[wall][:256])
    # axis-aligned rays lying exactly on voxel and brick faces, edges and through brick corners
    ijk = np.asarray(voxels[0], np.int64)
    ijk = ijk[:: max(1, ijk.shape[0] // 64)][:64]
    assert (ijk < 0).any() and (ijk > 0).any()
    brick = (ijk >> 3) << 3
    ao, ad = [], []
    for base in (ijk, brick, brick + 8):
        for off in ((0, 0, 0), (0.5, 0, 0), (0, 0.5, 0.5), (0.5, 0.5, 0.5)):
            for a in range(3):
                for s in (1.0, -1.0):
                    d = np.zeros(3)
                    d[a] = s
                    ao.append((base + np.array(off)) * vs - 1.5 * d)
                    ad.append(np.broadcast_to(d, base.shape))
    g["on_grid"] = (np.concatenate(ao), np.concatenate(ad))
    # rays near +-2^23 vs that leave the index domain, or enter it
    lim = float(1 << 23) * vs
    eo, ed = [], []
    for a in range(3):
        for s in (1.0, -1.0):
            for start in (lim - 1.0, lim - 0.05, lim + 1.0):
                for way in (1.0, -1.0):
                    o, d = np.zeros(3), np.zeros(3)
                    o[a] = s * start
                    d[a] = s * way
                    d[(a + 1) % 3] = 0.25
                    eo.append(o)
                    ed.append(d)
    g["domain_edge"] = (np.array(eo), np.array(ed))
    # a direction of length 1e30: off the map after one step
    g["huge_dir"] = (near[:32], d64[sel][:32] * 1e30)
    return g


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_edge_rays(maps, scan_rays, mode):
    m = maps["vdbfusion_f64"]
    groups = edge_rays(m.field, m.vol.export_voxels(), scan_rays)
    names = list(groups)
    o = np.ascontiguousarray(np.concatenate([groups[k][0] for k in names]).astype(F))
    d = np.ascontiguousarray(np.concatenate([groups[k][1] for k in names]).astype(F))
    ends = np.cumsum([groups[k][0].shape[0] for k in names])
    part = {k: slice(e - groups[k][0].shape[0], e) for k, e in zip(names, ends)}
    ref = rr.raycast(m.field, o, d, None, 0.0, 3.0, rr.STEP, MODES[mode])
    hit = ref[2].astype(bool)
    for k in names:
        print("%s %s: %d of %d hit" % (mode, k, hit[part[k]].sum(), hit[part[k]].size))
    # what the reference is expected to say
    for k in ("nonfinite", "zero_dir", "behind", "domain_edge", "huge_dir"):
        assert not hit[part[k]].any(), k
    assert groups["behind"][0].shape[0] >= 100
    s0 = sr.sample(m.field, o[part["behind"]], sr.NEAREST)
    assert (s0[3].astype(bool) & (s0[0] < 0)).mean() > 0.5  # they do start at S < 0
    near = hit[part["near"]]
    assert near.mean() >= (0.9 if mode == "nearest" else 0.2)
    assert np.abs(ref[0][part["near"]][near] - 1.5).max() < 0.2
    grid = hit[part["on_grid"]]
    assert grid.sum() >= 20 and (~grid).sum() >= 20
    assert_same(m.vol.raycast(o, d, None, 0.0, 3.0, rr.STEP, mode), ref)


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_degenerate_ranges(maps, scan_rays, mode):
    """t_min == t_max is one sample and never a hit; a [t_min, t_max] bracketing one step finds
    the crossing it brackets."""
    m = maps["vdbfusion_f64"]
    o, d = m.rays["scan"]
    ref = rr.raycast(m.field, o, d, None, 5.0, 5.0, rr.STEP, MODES[mode])
    assert rr.lattice(5.0, 5.0, rr.STEP).shape == (1,) and not ref[2].any()
    assert_same(m.vol.raycast(o, d, None, 5.0, 5.0, rr.STEP, mode), ref)
    # the lattice {t, t + step} around ray j's crossing
    full = m.reference("scan", mode, 0.0, rr.STEP)
    j = int(np.flatnonzero(full[2])[0])
    t = rr.lattice(rr.T_MIN, rr.T_MAX, rr.STEP)
    t0 = float(t[np.searchsorted(t, full[0][j], side="right") - 1])
    assert rr.lattice(t0, t0 + 1.5 * rr.STEP, rr.STEP).shape == (2,)
    ref = rr.raycast(m.field, o, d, None, t0, t0 + 1.5 * rr.STEP, rr.STEP, MODES[mode])
    assert ref[2][j] == 1 and abs(float(ref[0][j]) - float(full[0][j])) < 1e-3
    assert 1 <= ref[2].sum() < 2048
    assert_same(m.vol.raycast(o, d, None, t0, t0 + 1.5 * rr.STEP, rr.STEP, mode), ref)


GUARD = 8


def raycast_device(vol, o, d, mode, normals=True, **kw):
    """Through raw device pointers; the buffers carry GUARD elements past n."""
    import torch
    dev = vol.tensor_device
    n = d.shape[0]
    to = torch.from_numpy(np.ascontiguousarray(o, F).reshape(-1, 3)).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(d, F).reshape(-1, 3)).to(dev)
    depth = torch.full((n + GUARD,), -7.0, dtype=torch.float32, device=dev)
    normal = torch.full((n + GUARD, 3), -7.0, dtype=torch.float32, device=dev)
    hit = torch.full((n + GUARD,), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    vol.raycast_device(to.data_ptr() if n else None, td.data_ptr() if n else None, n,
                       depth.data_ptr(), normal.data_ptr() if normals else None, hit.data_ptr(),
                       mode=mode, **kw)
    return depth.cpu().numpy(), normal.cpu().numpy(), hit.cpu().numpy()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_small_counts_device_pointers(maps, n):
    """Partial waves; nothing is written past n; d_normal = NULL leaves the normals alone."""
    m = maps["vdbfusion_f64"]
    o, d = m.rays["scan"]
    pick = np.arange(n) * (2048 // 65)
    o, d = np.broadcast_to(o, d.shape)[pick], d[pick]
    kw = dict(t_min=rr.T_MIN, t_max=rr.T_MAX, step=rr.STEP)
    for mode in MODES:
        full = m.reference("scan", mode, 0.0, rr.STEP)
        ref = tuple(a[pick] for a in full)
        depth, normal, hit = raycast_device(m.vol, o, d, mode, **kw)
        assert_same((depth[:n], normal[:n], hit[:n]), ref)
        assert np.all(depth[n:] == -7) and np.all(normal[n:] == -7) and np.all(hit[n:] == 9)
        depth, normal, hit = raycast_device(m.vol, o, d, mode, normals=False, **kw)
        assert_same((depth[:n], None, hit[:n]), ref)
        assert np.all(normal == -7) and np.all(depth[n:] == -7) and np.all(hit[n:] == 9)


def test_device_past_the_grid_cap(maps, scans):
    """8192 * 256 + 77 rays: the last 77 are marched on a workgroup's second trip.  2039 distinct
    rays repeated (tests/pastcap.py), so the reference marches 2039 rays; 2039 does not divide
    the stride, so the ray one stride back is another one."""
    m = maps["vdbfusion_f64"]
    refs = pc.ray_references(m.field, scans[0])
    idx, rot = pc.ray_tiling(refs)
    sides = pc.ray_sides(refs, idx)
    print("rotation %d: %s" % (rot, sides))
    pc.assert_rays_past_cap(sides)
    o, d = pc.ray_distinct(scans[0])
    n = idx.size
    assert n == pc.RAY_N and np.all(idx[pc.RAY_STRIDE:] != idx[:n - pc.RAY_STRIDE])
    oo, dd = o[idx], d[idx]
    kw = dict(zip(("t_min", "t_max", "step"), pc.RAY_T))
    for mode in MODES:
        ref = tuple(a[idx] for a in refs[mode])
        depth, normal, hit = raycast_device(m.vol, oo, dd, mode, **kw)
        assert_same((depth[:n], normal[:n], hit[:n]), ref)
        assert np.all(depth[n:] == -7) and np.all(normal[n:] == -7) and np.all(hit[n:] == 9)


def test_two_calls_give_the_same_bits(maps):
    m = maps["voxblox"]
    o, d = m.rays["displaced"]
    kw = dict(t_min=rr.T_MIN, t_max=rr.T_MAX, step=0.03)
    for mode in MODES:
        a = raycast_device(m.vol, np.broadcast_to(o, d.shape), d, mode, **kw)
        b = raycast_device(m.vol, np.broadcast_to(o, d.shape), d, mode, **kw)
        assert a[2][:-GUARD].sum() >= 100
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_host_entry_point_works_in_pieces(scans, scan_rays):
    """tsdf_raycast on n = 3 max_points / 2 rays (two pieces) equals tsdf_raycast_device on them
    and the reference."""
    from tsdf_map import HipTSDFVolume
    pts, org = scans[0]
    o, d, _ = scan_rays
    with HipTSDFVolume(VS, TAU, max_points=2048) as v:
        for k in range(0, pts.shape[0], 2048):  # the whole scan, a column block at a time
            v.integrate(pts[k:k + 2048], org)
        n = 3 * 2048 // 2
        dd = np.ascontiguousarray(np.concatenate([d, d[::2]])[:n])
        oo = np.broadcast_to(o, dd.shape).copy()
        oo[2048:] += np.array(rr.DISPLACED, F)
        kw = dict(t_min=rr.T_MIN, t_max=rr.T_MAX, step=rr.STEP)
        for mode in MODES:
            ref = rr.raycast(sr.field_of(v), oo, dd, None, mode=MODES[mode], **kw)
            assert ref[2][:2048].sum() >= 10 and ref[2][2048:].sum() >= 10
            assert_same(v.raycast(oo, dd, mode=mode, **kw), ref)
            depth, normal, hit = raycast_device(v, oo, dd, mode, **kw)
            assert_same((depth[:n], normal[:n], hit[:n]), ref)


def test_raycast_flushes_the_pending_scan(scans, scan_rays):
    from tsdf_map import HipTSDFVolume
    pts, org = scans[0]
    o, d, _ = scan_rays
    with HipTSDFVolume(VS, TAU) as v:
        empty = v.raycast(o, d[:256], t_max=rr.T_MAX)
        assert not empty[2].any() and not empty[0].any() and not empty[1].any()
        v.integrate(pts, org)  # queued
        got = v.raycast(o, d[:256], t_min=rr.T_MIN, t_max=rr.T_MAX)  # nearest, step = voxel / 2
        ref = rr.raycast(sr.field_of(v), o, d[:256], None, rr.T_MIN, rr.T_MAX, VS / 2)
        assert ref[2].sum() >= 200
        assert_same(got, ref)


def test_arguments_are_checked(maps):
    from tsdf_map import HipTSDFVolume, TsdfError, _abi
    m = maps["vdbfusion_f64"]
    v, lib = m.vol, m.vol._lib
    one = C.c_void_p(8)  # never dereferenced: the arguments are refused first
    nan, inf = float("nan"), float("inf")

    def dev(org=one, dirs=one, n=64, t_min=0.0, t_max=10.0, step=0.05, mode=0, mw=0.0, depth=one,
            hit=one):
        return lib.tsdf_raycast_device(v._ctx, org, dirs, n, None, t_min, t_max, step, mode, mw,
                                       depth, None, hit)

    bad = ({"mode": 2}, {"mode": -1}, {"mw": -1.0}, {"mw": nan}, {"org": None}, {"dirs": None},
           {"depth": None}, {"hit": None}, {"step": 0.0}, {"step": -0.05}, {"step": nan},
           {"step": inf}, {"t_min": -0.5}, {"t_min": nan}, {"t_max": inf}, {"t_max": nan},
           {"t_min": 2.0, "t_max": 1.0}, {"t_max": 1e6, "step": 0.5},
           {"t_min": 0.0, "t_max": 1.0, "step": 2.0 ** -20})
    for kw in bad:
        assert dev(**kw) == _abi.TSDF_EINVAL, kw
        assert lib.tsdf_last_error(v._ctx), kw
    assert dev(n=0, org=None, dirs=None, depth=None, hit=None) == _abi.TSDF_OK
    # the host entry point applies the same rules
    o = np.zeros((4, 3), F)
    fp = lambda a: a.ctypes.data_as(_abi.FP)  # noqa: E731
    depth, hit = np.empty(4, F), np.empty(4, np.uint8)
    u8 = hit.ctypes.data_as(_abi.U8P)
    assert lib.tsdf_raycast(v._ctx, fp(o), fp(o), 4, None, 0.0, 1.0, 0.05, 0, 0.0, fp(depth), None,
                            u8) == _abi.TSDF_OK
    for args in ((None, fp(o), 4, None, 0.0, 1.0, 0.05, 0, 0.0, fp(depth), None, u8),
                 (fp(o), fp(o), 4, None, 0.0, 1.0, 0.05, 0, 0.0, None, None, u8),
                 (fp(o), fp(o), 4, None, 0.0, 1.0, 0.05, 0, 0.0, fp(depth), None, None),
                 (fp(o), fp(o), 4, None, 0.0, 1.0, 0.0, 0, 0.0, fp(depth), None, u8),
                 (fp(o), fp(o), 4, None, 1.0, 0.5, 0.05, 0, 0.0, fp(depth), None, u8),
                 (fp(o), fp(o), 4, None, 0.0, 1.0, 0.05, 3, 0.0, fp(depth), None, u8)):
        assert lib.tsdf_raycast(v._ctx, *args) == _abi.TSDF_EINVAL, args
    with pytest.raises(ValueError):
        v.raycast(o[0], o, mode="cubic")
    with pytest.raises(TsdfError) as e:
        v.raycast(o[0], o, step=0.0)
    assert e.value.code == _abi.TSDF_EINVAL and "step" in str(e.value)
    with pytest.raises(TsdfError) as e:
        v.raycast(o[0], o, t_min=3.0, t_max=2.0)
    assert e.value.code == _abi.TSDF_EINVAL and "t_min" in str(e.value)
    # a sector shard of the map is refused
    with HipTSDFVolume(VS, TAU, n_sectors=2, sector=0) as sh:
        with pytest.raises(TsdfError) as e:
            sh.raycast(o[0], o)
        assert e.value.code == _abi.TSDF_EINVAL and "n_sectors" in str(e.value)


def test_range_image(maps, scan_rays):
    """A 16 x 64 image equals a direct raycast of its rays."""
    from tsdf_map import render
    m = maps["vdbfusion_f64"]
    org = scan_rays[0]
    rays = render.spherical_rays(16, 64, np.deg2rad(-20.0), np.deg2rad(15.0))
    assert rays.shape == (1024, 3)
    T = np.eye(4)
    T[:3, :3] = sr.exp_so3([0.0, 0.0, 1.1])
    T[:3, 3] = org
    kw = dict(t_min=rr.T_MIN, t_max=rr.T_MAX, step=rr.STEP, mode="nearest")
    depth, hit = render.range_image(m.vol, T, rays, shape=(16, 64), **kw)
    assert depth.shape == (16, 64) and hit.shape == (16, 64) and depth.dtype == F
    d, _, h = m.vol.raycast(np.zeros(3, F), rays, pose=T, normals=False, **kw)
    assert np.array_equal(bits(depth), bits(d.reshape(64, 16).T)) and np.array_equal(
        hit, h.reshape(64, 16).T)
    ref = rr.raycast(m.field, np.zeros(3, F), rays, T[:3], rr.T_MIN, rr.T_MAX, rr.STEP)
    assert ref[2].sum() >= 500
    assert np.array_equal(bits(d), bits(ref[0])) and np.array_equal(h, ref[2].astype(bool))
    flat_depth, flat_hit = render.range_image(m.vol, T, rays, **kw)
    assert np.array_equal(bits(flat_depth), bits(d)) and np.array_equal(flat_hit, h)
