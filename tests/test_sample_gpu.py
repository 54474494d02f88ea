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


# ---- the align sums and k_sample at the counts that break reductions ------------------------------

ALIGN_CAP = 1024 * 256        # ALIGN_MAX_WG workgroups of 256 lanes: one pass of k_align
N_LONG = ALIGN_CAP + 321      # ... and 321 points of a second pass
N_PAST_GRID = 8192 * 256 + 77  # past k_sample's grid cap
COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 1000]


def words(H, b, e, nv):
    """The 44 output words: H row-major, b, e, n_valid."""
    return np.concatenate([np.asarray(H, np.float64).reshape(36), b, [e, nv]])


def check_align(m, pts, pose, mw=0.0, got=None):
    """n_valid exactly; each of the 43 sums within n_valid 2^-52 sum|term| of the reference's
    double sum, the bound of any summation order of the same double terms (the kernel forms each
    term in double from the same fp32 values); with at most one term there is nothing to reorder,
    and the sums must be equal.  Returns (the 44 words, n_valid)."""
    H, b, e, nv, ab = sr.align_terms(m.field, pts, pose, mw)
    if got is None:
        got = m.vol.align_terms(pts, pose, mw)
    g, ref = words(*got), words(H, b, e, nv)
    assert got[3] == nv
    err = np.abs(g[:43] - ref[:43])
    if nv <= 1:
        assert np.array_equal(g, ref)
    else:
        tol = nv * 2.0 ** -52 * ab[:43]
        assert np.all(err <= tol), (err / tol).max()
    assert np.array_equal(got[0], got[0].T)
    return g, nv


def slice_with(valid, n):
    """The start of the first run of n consecutive queries that has a valid one (n = 1), exactly
    one valid and one invalid (n = 2), or at least one of each."""
    c = np.concatenate([[0], np.cumsum(valid.astype(np.int64))])
    k = c[n:] - c[:-n]  # valid ones in [i, i + n)
    ok = (k == 1) if n <= 2 else (k >= 1) & (k < n)
    return int(np.argmax(ok)) if ok.any() else None


def far(pts):
    """The same points 1000 m away: no map there, every sample invalid."""
    return np.ascontiguousarray(np.asarray(pts, F) + F(1000.0))


@pytest.fixture(scope="module")
def long_cloud(sim, scan0):
    """N_LONG points: scans 0, 1 and 2 concatenated and cut (two scans hold 262 144 points at the
    most, one short of a second pass)."""
    p = np.concatenate([scan0[0], sim.scan(1)[0], sim.scan(2)[0]])
    assert p.shape[0] >= N_LONG
    return np.ascontiguousarray(p[:N_LONG])


@pytest.mark.parametrize("n", COUNTS)
def test_align_counts(maps, queries, n):
    """A lane alone, partial waves, a partial workgroup, whole ones and one lane more."""
    m = maps["vdbfusion_f64"]
    pose = sr.start_pose()
    valid = sr.sample(m.field, sr.transform(pose, queries), sr.TRILINEAR)[3].astype(bool)
    k0 = slice_with(valid, n)
    assert k0 is not None
    pts = np.ascontiguousarray(queries[k0:k0 + n])
    g, nv = check_align(m, pts, pose)
    assert (nv == 1) if n <= 2 else (1 <= nv < n)
    print("n %d at %d: n_valid %d" % (n, k0, nv))
    if n == 257:  # the same bits on every call
        assert np.array_equal(words(*m.vol.align_terms(pts, pose)).view(np.uint64),
                              g.view(np.uint64))


def test_align_no_valid_point(maps, queries):
    m = maps["vdbfusion_f64"]
    for n in (1, 300, 5000):
        g, nv = check_align(m, far(queries[:n]), sr.start_pose())
        assert nv == 0 and not g.view(np.uint64).any()  # all 44 words exactly +0


def test_align_only_the_last_of_300_is_valid(maps, queries):
    """One workgroup and a wave of the next without a valid point, then a lone valid lane."""
    m = maps["vdbfusion_f64"]
    pose = np.eye(4)[:3]
    valid = m.reference(queries, "trilinear", 0.0)[3].astype(bool)
    pts = far(queries[:300])
    pts[299] = queries[np.argmax(valid)]
    g, nv = check_align(m, pts, pose)
    assert nv == 1 and g[42] > 0


def test_align_second_pass(maps, long_cloud):
    """More points than ALIGN_MAX_WG x 256: 321 lanes accumulate over two passes.  Then the same
    cloud with every point of the first pass made invalid, so that only second-pass lanes hold
    anything; and the same bits on every call."""
    m = maps["vdbfusion_f64"]
    pose = sr.start_pose()
    g, nv = check_align(m, long_cloud, pose)
    tail = check_align(m, long_cloud[ALIGN_CAP:], pose)[1]
    print("long cloud: n_valid %d, %d of them in the second pass" % (nv, tail))
    assert nv >= 1000 and tail >= 10
    assert np.array_equal(words(*m.vol.align_terms(long_cloud, pose)).view(np.uint64),
                          g.view(np.uint64))
    only = long_cloud.copy()
    only[:ALIGN_CAP] = far(only[:ALIGN_CAP])
    g2, nv2 = check_align(m, only, pose)
    assert nv2 == tail and g2[42] > 0


def test_align_on_the_voxblox_map(maps, scan0):
    """Background 0 instead of tau."""
    m = maps["voxblox"]
    pts = np.ascontiguousarray(scan0[0][::8])
    g, nv = check_align(m, pts, sr.start_pose())
    print("voxblox: n_valid %d" % nv)
    assert nv >= 1000


def test_align_device_pointer_unaligned(maps, scan0):
    """The device-pointer form on points 12 bytes into an allocation (not 16-byte aligned)."""
    import torch
    m = maps["vdbfusion_f64"]
    pts = np.ascontiguousarray(scan0[0][::8][:4099])
    pose = sr.start_pose()
    g, nv = check_align(m, pts, pose)
    assert nv >= 100
    d = torch.full((pts.shape[0] + 2, 3), 1000.0, dtype=torch.float32, device=m.vol.tensor_device)
    d[1:-1] = torch.from_numpy(pts).to(d.device)
    torch.cuda.synchronize(d.device)
    ptr = d.data_ptr() + 12
    assert d.data_ptr() % 16 == 0 and ptr % 16 != 0
    got = m.vol.align_terms(ptr, pose, n=pts.shape[0])
    assert np.array_equal(words(*got).view(np.uint64), g.view(np.uint64))


def tiled_queries(points, origin, n):
    """n queries: the scan's query points (every 8th with range > 0.5 m) tiled, each tile with a
    fresh seeded +-5 cm jitter."""
    q = np.asarray(points, F)[::8]
    rng_m = np.linalg.norm(q.astype(np.float64) - np.asarray(origin, np.float64), axis=1)
    q = q[rng_m > 0.5]
    tiles = []
    for t in range(-(-n // q.shape[0])):
        jit = np.random.default_rng(1000 + t).uniform(-0.05, 0.05, q.shape)
        tiles.append((q + jit).astype(F))
    return np.ascontiguousarray(np.concatenate(tiles)[:n])


def test_sample_device_past_the_grid_cap(maps, scan0):
    """More queries than 8192 x 256: 77 lanes of k_sample run the loop body twice."""
    m = maps["vdbfusion_f64"]
    q = tiled_queries(*scan0, N_PAST_GRID)
    assert q.shape[0] == N_PAST_GRID
    ref = sr.sample(m.field, q, sr.TRILINEAR)
    share = ref[3].mean()
    print("past the grid cap: %.1f %% valid, %d of the last 77" % (100 * share, ref[3][-77:].sum()))
    assert 0.30 <= share <= 0.60 and 0 < ref[3][-77:].sum() < 77
    assert_same(sample_device(m.vol, q, "trilinear"), ref)
