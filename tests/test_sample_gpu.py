"""Sparse map queries on the GPU (include/tsdf_hip_sample.h) against tests/sampleref.py, bit for
bit: the reference reads the GPU context's own export_voxels(), which is bitwise the oracle's, so
what test_sample_ref.py pins on the CPU is what the kernels are held to here."""
import ctypes as C

import numpy as np
import pytest

import sampleref as sr

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"nearest": sr.NEAREST, "trilinear": sr.TRILINEAR}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same(got, ref):
    """(sdf, weight, grad, valid) of the library against the reference's, bitwise."""
    gs, gw, gg, gv = got
    rs, rw, rg, rv = ref
    assert np.array_equal(np.asarray(gv).astype(np.uint8), rv)
    assert np.array_equal(bits(gs), bits(rs))
    assert np.array_equal(bits(gw), bits(rw))
    assert np.array_equal(bits(gg), bits(rg))


class Map:
    def __init__(self, vol):
        self.vol = vol
        self.field = sr.field_of(vol)
        self.ref = {}

    def reference(self, queries, mode, mw):
        """The reference samples of the shared queries, computed once per (mode, min_weight)."""
        k = (mode, mw)
        if k not in self.ref:
            self.ref[k] = sr.sample(self.field, queries, MODES[mode], mw)
        return self.ref[k]


@pytest.fixture(scope="module")
def queries(scan0):
    return sr.jitter_queries(*scan0)


@pytest.fixture(scope="module")
def maps(scan0):
    from tsdf_map import HipTSDFVolume
    pts, org = scan0
    assert pts.shape[0] == 131072
    out = {}
    for sem, p in (("vdbfusion_f64", pts), ("voxblox", np.ascontiguousarray(pts[::2]))):
        v = HipTSDFVolume(sr.VOXEL_SIZE, sr.SDF_TRUNC, semantics=sem)
        v.integrate(p, org)
        v.sync()
        out[sem] = Map(v)
    assert out["voxblox"].field.bg == 0 and out["vdbfusion_f64"].field.bg == F(sr.SDF_TRUNC)
    yield out
    for m in out.values():
        m.vol.close()


def not_vacuous(m, sem, queries):
    """The conditions every comparison asserts on the reference (trilinear, min_weight 0)."""
    v = m.reference(queries, "trilinear", 0.0)[3]
    if sem == "voxblox":
        assert v.sum() >= 1000
    else:
        sr.check_not_vacuous(m.field, queries, v)


@pytest.mark.parametrize("min_weight", [0.0, 2.0])
@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_sample_bitwise(maps, queries, sem, mode, min_weight):
    m = maps[sem]
    not_vacuous(m, sem, queries)
    ref = m.reference(queries, mode, min_weight)
    got = m.vol.sample(queries, mode=mode, min_weight=min_weight)
    print("%s %s min_weight %g: %d of %d valid" % (sem, mode, min_weight, ref[3].sum(), ref[3].size))
    assert ref[3].sum() >= 100
    assert_same(got, ref)


def edge_points(field, voxels):
    """Non-finite points, the index domain's border, and points on voxel and brick faces, edges
    and corners around observed voxels (negative coordinates included)."""
    vs = float(field.vs)
    lim = float(1 << 23)
    special = [[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0], [0, -np.inf, 0],
               [0, 0, np.inf], [-np.inf, np.inf, np.nan]]
    for a in range(3):
        for s in (1.0, -1.0):
            for k in (lim, lim - 1, lim - 2, lim + 1, 2 * lim, lim - 0.5, lim - 1.5, 1e30, 3e38):
                p = [0.0, 0.0, 0.0]
                p[a] = s * k * vs
                special.append(p)
    ijk = np.asarray(voxels[0], np.int64)
    ijk = ijk[:: max(1, ijk.shape[0] // 256)][:256]
    assert (ijk < 0).any() and (ijk > 0).any()
    brick = (ijk >> 3) << 3
    offs = [(0, 0, 0), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5), (0.5, 0.5, 0), (0, 0.5, 0.5),
            (0.5, 0, 0.5), (0.5, 0.5, 0.5), (1, 1, 1), (0.25, 0.75, 0.5)]
    on_grid = [(base + np.array(o)) * vs for base in (ijk, brick, brick + 7, brick + 7.5)
               for o in offs]
    return np.ascontiguousarray(np.concatenate([np.array(special)] + on_grid).astype(F))


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_edge_cases(maps, mode):
    m = maps["vdbfusion_f64"]
    p = edge_points(m.field, m.vol.export_voxels())
    ref = sr.sample(m.field, p, MODES[mode])
    v = ref[3].astype(bool)
    assert v.sum() > 100 and (~v).sum() > 100
    assert not v[:7].any() and np.all(ref[0][:7] == m.field.bg) and not ref[1][:7].any()
    assert_same(m.vol.sample(p, mode=mode), ref)


def sample_device(vol, pts, mode, min_weight=0.0, grad=True):
    import torch
    dev = vol.tensor_device
    n = pts.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(pts, F)).to(dev)
    s = torch.full((max(n, 1),), -7.0, dtype=torch.float32, device=dev)
    w = torch.full((max(n, 1),), -7.0, dtype=torch.float32, device=dev)
    g = torch.full((max(n, 1), 3), -7.0, dtype=torch.float32, device=dev)
    v = torch.full((max(n, 1),), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    vol.sample_device(d.data_ptr(), n, s.data_ptr(), w.data_ptr(), g.data_ptr() if grad else None,
                      v.data_ptr(), mode=mode, min_weight=min_weight)
    return s.cpu().numpy(), w.cpu().numpy(), g.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_small_counts_device_pointers(maps, queries, n):
    """The device entry point through torch tensors; partial waves; d_grad = NULL leaves the
    gradient buffer alone; nothing is written past n."""
    m = maps["vdbfusion_f64"]
    q = queries[-4096:][:: 4096 // 65][:n] if n else queries[:0]
    for mode in MODES:
        ref = sr.sample(m.field, q, MODES[mode])
        s, w, g, v = sample_device(m.vol, q, mode)
        assert_same((s[:n], w[:n], g[:n], v[:n]), ref)
        assert np.all(s[n:] == -7) and np.all(w[n:] == -7) and np.all(g[n:] == -7)
        assert np.all(v[n:] == 9)
        s, w, g, v = sample_device(m.vol, q, mode, grad=False)
        assert np.array_equal(bits(s[:n]), bits(ref[0])) and np.array_equal(v[:n], ref[3])
        assert np.all(g == -7)


def test_device_entry_point_full_cloud(maps, queries):
    m = maps["vdbfusion_f64"]
    not_vacuous(m, "vdbfusion_f64", queries)
    for mode, mw in (("trilinear", 0.0), ("nearest", 2.0)):
        assert_same(sample_device(m.vol, queries, mode, mw), m.reference(queries, mode, mw))


def test_host_layouts(maps, queries):
    """dlio::Point-style records (point_step 32, xyz at offset 0, fp32) and packed float64."""
    m = maps["vdbfusion_f64"]
    not_vacuous(m, "vdbfusion_f64", queries)
    q = queries[:4096]
    ref = tuple(a[:4096] for a in m.reference(queries, "trilinear", 0.0))
    rec = np.zeros((q.shape[0], 8), F)
    rec[:, :3] = q
    rec[:, 3:] = 1e9  # the rest of the record is not coordinates
    assert_same(m.vol.sample_cloud(rec.tobytes(), q.shape[0], 32, 0), ref)
    rec2 = np.full((q.shape[0], 8), 1e9, F)  # ... nor is what precedes them
    rec2[:, 2:5] = q
    assert_same(m.vol.sample_cloud(rec2.tobytes(), q.shape[0], 32, 8), ref)
    # float64 coordinates are rounded to fp32: perturb below half an ulp
    q64 = q.astype(np.float64) * (1.0 + 1e-9)
    assert q64.dtype == np.float64 and np.array_equal(q64.astype(F), q)
    assert_same(m.vol.sample(q64), ref)


def test_larger_than_max_points_is_looped(scan0, queries):
    from tsdf_map import HipTSDFVolume
    pts, org = scan0
    with HipTSDFVolume(sr.VOXEL_SIZE, sr.SDF_TRUNC, max_points=5000) as v:
        v.integrate(pts[:5000], org)
        field = sr.field_of(v)
        q = queries[:12001]
        ref = sr.sample(field, q, sr.NEAREST)
        assert ref[3].sum() > 10
        assert_same(v.sample(q, mode="nearest"), ref)


def test_sample_flushes_the_pending_scan(scan0, queries):
    """integrate without sync, then sample: the queued scan is in the answer."""
    from tsdf_map import HipTSDFVolume
    pts, org = scan0
    with HipTSDFVolume(sr.VOXEL_SIZE, sr.SDF_TRUNC) as v:
        q = queries[:2048]
        empty = v.sample(q)
        assert not empty[3].any() and np.all(empty[0] == F(sr.SDF_TRUNC))
        v.integrate(pts, org)  # queued: the batch holds one scan of max_batch
        got = v.sample(q)
        H, b, e, nv = v.align_terms(q, np.eye(4))
        field = sr.field_of(v)
        ref = sr.sample(field, q, sr.TRILINEAR)
        assert ref[3].sum() > 500
        assert_same(got, ref)
        assert nv == ref[3].sum()


def test_arguments_are_checked(maps, queries):
    from tsdf_map import HipTSDFVolume, TsdfError, _abi
    m = maps["vdbfusion_f64"]
    v, lib = m.vol, m.vol._lib
    q = np.ascontiguousarray(queries[:64])
    s, w, g = np.empty(64, F), np.empty(64, F), np.empty((64, 3), F)
    val = np.empty(64, np.uint8)
    fp = lambda a: a.ctypes.data_as(_abi.FP)  # noqa: E731
    u8 = val.ctypes.data_as(C.POINTER(C.c_uint8))
    qp = q.ctypes.data_as(C.c_void_p)

    def host(mode=1, mw=0.0, pts=qp, sdf=fp(s), wt=fp(w), vd=u8, step=12, off=0, n=64):
        return lib.tsdf_sample(v._ctx, pts, n, step, off, 0, mode, mw, sdf, wt, fp(g), vd)

    assert host() == _abi.TSDF_OK
    for kw in ({"mode": 2}, {"mode": -1}, {"mw": -1.0}, {"mw": float("nan")}, {"pts": None},
               {"sdf": None}, {"wt": None}, {"vd": None}, {"step": 8}, {"step": 16, "off": 8}):
        assert host(**kw) == _abi.TSDF_EINVAL, kw
        assert lib.tsdf_last_error(v._ctx), kw
    assert host(n=0, pts=None, sdf=None, wt=None, vd=None) == _abi.TSDF_OK
    one = C.c_void_p(8)  # never dereferenced: the arguments are refused first
    for args in ((None, 64, 1, 0.0, one, one, None, one), (one, 64, 1, 0.0, None, one, None, one),
                 (one, 64, 1, 0.0, one, None, None, one), (one, 64, 1, 0.0, one, one, None, None),
                 (one, 64, 7, 0.0, one, one, None, one), (one, 64, 1, -0.5, one, one, None, one),
                 (one, 64, 1, float("nan"), one, one, None, one)):
        assert lib.tsdf_sample_device(v._ctx, *args) == _abi.TSDF_EINVAL, args
    assert lib.tsdf_sample_device(v._ctx, None, 0, 1, 0.0, None, None, None, None) == _abi.TSDF_OK
    pose = np.eye(4)[:3].copy()
    out = np.empty(44)
    d3 = lambda a: a.ctypes.data_as(_abi.D3)  # noqa: E731
    assert lib.tsdf_align_terms_device(v._ctx, one, 64, None, 0.0, d3(out)) == _abi.TSDF_EINVAL
    assert lib.tsdf_align_terms_device(v._ctx, one, 64, d3(pose), 0.0, None) == _abi.TSDF_EINVAL
    assert lib.tsdf_align_terms_device(v._ctx, None, 64, d3(pose), 0.0, d3(out)) == _abi.TSDF_EINVAL
    assert lib.tsdf_align_terms_device(v._ctx, one, 64, d3(pose), -1.0, d3(out)) == _abi.TSDF_EINVAL
    assert lib.tsdf_align_terms_device(v._ctx, None, 0, d3(pose), 0.0, d3(out)) == _abi.TSDF_OK
    assert not out.any()
    with pytest.raises(ValueError):
        v.sample(q, mode="cubic")
    # a sector shard of the map is refused: sampling it needs a halo exchange
    with HipTSDFVolume(sr.VOXEL_SIZE, sr.SDF_TRUNC, n_sectors=2, sector=0) as sh:
        with pytest.raises(TsdfError) as e:
            sh.sample(q)
        assert e.value.code == _abi.TSDF_EINVAL and "n_sectors" in str(e.value)
        with pytest.raises(TsdfError) as e:
            sh.align_terms(q, np.eye(4))
        assert e.value.code == _abi.TSDF_EINVAL


def test_align_terms_match_the_reference(maps, scan0):
    """n_valid exactly; every sum within n_valid 2^-52 sum|term| of the reference's double sum (the
    bound of any summation order of the same double terms); and the same bits on every call."""
    m = maps["vdbfusion_f64"]
    pts = np.ascontiguousarray(scan0[0][::8])
    for pose, mw in ((sr.start_pose(), 0.0), (np.eye(4)[:3], 2.0)):
        H, b, e, nv, ab = sr.align_terms(m.field, pts, pose, mw)
        assert nv > 1000
        gH, gb, ge, gnv = m.vol.align_terms(pts, pose, mw)
        assert gnv == nv
        got = np.concatenate([gH.reshape(36), gb, [ge]])
        ref = np.concatenate([H.reshape(36), b, [e]])
        tol = nv * 2.0 ** -52 * ab[:43]
        err = np.abs(got - ref)
        print("min_weight %g: n_valid %d, max err / tol = %.3g" % (mw, nv, (err / tol).max()))
        assert np.all(err <= tol), (err / tol).max()
        assert np.array_equal(gH, gH.T)
        again = m.vol.align_terms(pts, pose, mw)
        assert np.array_equal(again[0].view(np.uint64), gH.view(np.uint64))
        assert np.array_equal(again[1].view(np.uint64), gb.view(np.uint64))
        assert again[2] == ge and again[3] == gnv


def test_refine_pose(maps, scan0):
    """The CPU suite's Gauss-Newton check (test_sample_ref.py), through the fused kernel."""
    from tsdf_map import align
    m = maps["vdbfusion_f64"]
    pts = np.ascontiguousarray(scan0[0][::8])
    T, steps = align.refine_pose(m.vol, pts, sr.start_pose(), iters=6)
    for k, st in enumerate(steps):
        print("step %d: rms %.4f m, n_valid %d" % (k, st["rms"], st["n_valid"]))
    t, a = sr.pose_error(T)
    print("after 6 steps: |t| = %.3f cm, angle = %.4f deg" % (100 * t, a))
    assert len(steps) == 6 and t < 0.01 and a < 0.1
    assert steps[-1]["rms"] < steps[0]["rms"]
    _, _, e, nv = m.vol.align_terms(pts, T)
    assert np.sqrt(e / nv) < steps[0]["rms"]
    with pytest.raises(align.AlignError):
        align.refine_pose(m.vol, pts[:4] + 1000.0, np.eye(4))
