"""What the read-out and exchange entry points of libtsdf_hip.so refuse, and what they report when
they do: the status code, the text of tsdf_last_error and the count, through the C entry points of
the loaded library, each on a map of three imported bricks.  After a refusal the same call with
good arguments must give what the oracle gives, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from test_multigpu import emulated_reduce_host, voxels_equal_bitwise
from tsdf_map import HipTSDFVolume, _abi, border_reduce_local

pytestmark = pytest.mark.gpu

VS, TAU = 0.05, 0.15
SMALL = dict(max_bricks=1 << 12, max_points=1 << 12, max_batch=4)
COORDS = [(0, 0, 1), (1, 0, 0), (-1, 1, 0)]  # not in (z, y, x) order
ZYX = [(1, 0, 0), (-1, 1, 0), (0, 0, 1)]
LO, HI = -(1 << 20), (1 << 20) - 1  # the brick coordinates a key holds
SHARDED = ("%s: the context holds one sector shard of the map (n_sectors > 1); %s a sharded field is "
           "not supported")
MODE = "%s: mode must be TSDF_SAMPLE_NEAREST or _TRILINEAR"
WEIGHT = "%s: min_weight is negative or NaN"


def bricks(coords, seed=0):
    """A slanted plane through the given bricks, with unobserved voxels scattered in it."""
    c = np.asarray(coords, np.int32).reshape(-1, 3)
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    g = [8 * c[:, a, None, None, None] + v[None] for a, v in enumerate((x, y, z))]
    s = np.clip(VS * (0.6 * g[0] + 0.3 * g[1] + 0.5 * g[2]) - 0.35 + 0.01 * seed, -TAU, TAU)
    w = np.random.default_rng(seed).integers(0, 16, s.shape)
    return c, s.astype(np.float32), w.astype(np.float32)


def text(v):
    return v._lib.tsdf_last_error(v._ctx).decode()


def refused(v, rc, code, msg):
    assert rc == code and text(v) == msg, (rc, text(v))


def same_bricks(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def maps():
    """(the GPU map, its oracle twin) of three bricks; the tests that use it only read."""
    g, o = HipTSDFVolume(VS, TAU, **SMALL), oracle.OracleTSDFVolume(VS, TAU)
    for v in (g, o):
        v.import_bricks(*bricks(COORDS))
    yield g, o
    g.close()


def test_export_bricks_cap(maps):
    g, o = maps
    c = np.zeros((3, 3), np.int32)
    s = np.zeros((3, 8, 8, 8), np.float32)
    w = np.zeros_like(s)
    n = C.c_uint64()

    def export(cap):
        return g._lib.tsdf_export_bricks(g._ctx, c.ctypes.data_as(_abi.I3), s.ctypes.data_as(_abi.FP),
                                         w.ctypes.data_as(_abi.FP), cap, C.byref(n))

    refused(g, export(2), _abi.TSDF_EOVERFLOW, "export needs 3 bricks")
    assert n.value == 3
    assert export(3) == _abi.TSDF_OK and n.value == 3
    assert c.tolist() == [list(b) for b in ZYX]
    assert same_bricks((c, s, w), o.export_bricks())


def test_extract_mesh_cap(maps):
    g, o = maps
    want = o.extract_triangle_mesh()[0]
    nt = want.shape[0] // 3
    assert nt > 50
    tri = np.zeros((nt, 9), np.float32)
    n = C.c_uint64()

    def mesh(cap):
        return g._lib.tsdf_extract_mesh_table(g._ctx, 0.0, _abi.MC_TABLES["generated"],
                                              tri.ctypes.data_as(_abi.FP), cap, C.byref(n))

    refused(g, mesh(nt - 1), _abi.TSDF_EOVERFLOW, "mesh has %d triangles" % nt)
    assert n.value == nt
    assert mesh(nt) == _abi.TSDF_OK and n.value == nt
    assert np.array_equal(tri.reshape(-1, 3).view(np.uint32), want.view(np.uint32))


def test_brick_keys_cap(maps):
    g, _ = maps
    k = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    n = C.c_uint64()
    rc = g._lib.tsdf_brick_keys_device(g._ctx, C.c_void_p(k.data_ptr()), 2, C.byref(n))
    refused(g, rc, _abi.TSDF_EOVERFLOW, "brick keys need 3 entries")
    assert n.value == 3


def test_query_dense_bounds(maps):
    g, _ = maps

    def query(lo, hi):
        lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
        return g._lib.tsdf_query_dense(g._ctx, lo.ctypes.data_as(_abi.L3), hi.ctypes.data_as(_abi.L3),
                                       None, None)

    refused(g, query([0, 0, 0], [8, -1, 8]), _abi.TSDF_EINVAL, "hi < lo")
    refused(g, query([0, -(1 << 30), 0], [8, 1 << 30, 8]), _abi.TSDF_EINVAL,
            "query extent >= 2^31 voxels")
    # the first axis at fault decides
    refused(g, query([0, 0, 9], [1 << 31, 8, 8]), _abi.TSDF_EINVAL, "query extent >= 2^31 voxels")


def test_import_bricks_refusals():
    g, o = HipTSDFVolume(VS, TAU, **SMALL), oracle.OracleTSDFVolume(VS, TAU)
    for v in (g, o):
        v.import_bricks(*bricks(COORDS))

    def load(coords, seed):
        c, s, w = bricks(coords, seed)
        return g._lib.tsdf_import_bricks(g._ctx, c.ctypes.data_as(_abi.I3), s.ctypes.data_as(_abi.FP),
                                         w.ctypes.data_as(_abi.FP), c.shape[0])

    refused(g, load(COORDS + [COORDS[1]], 1), _abi.TSDF_EINVAL, "duplicate brick in import")
    for bad in (HI + 1, LO - 1):
        for axis in range(3):
            b = [0, 0, 0]
            b[axis] = bad
            refused(g, load(COORDS + [tuple(b)], 1), _abi.TSDF_EINVAL, "brick coordinate out of range")
    # the range rule is checked for every brick before the duplicates are looked for
    refused(g, load([COORDS[0], COORDS[0], (0, HI + 1, 0)], 1), _abi.TSDF_EINVAL,
            "brick coordinate out of range")
    assert g.num_bricks() == 3 and same_bricks(g.export_bricks(), o.export_bricks())
    edge = [(LO, 0, HI), (0, LO, 0)]  # the ends of the range are inside it
    assert load(edge, 2) == _abi.TSDF_OK, text(g)
    assert load(COORDS, 3) == _abi.TSDF_OK, text(g)  # a merge into the bricks held
    o.import_bricks(*bricks(edge, 2))
    o.import_bricks(*bricks(COORDS, 3))
    assert g.num_bricks() == 5 and same_bricks(g.export_bricks(), o.export_bricks())
    g.close()


@pytest.fixture(scope="module")
def shard():
    """One sector shard of two, which neither samples nor raycasts."""
    g = HipTSDFVolume(VS, TAU, n_sectors=2, sector=0, **SMALL)
    g.import_bricks(*bricks(COORDS))
    yield g
    g.close()


def sample_call(v, mode, min_weight):
    p = np.zeros((4, 3), np.float32)
    s, w, g, ok = np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(12, np.float32), \
        np.zeros(4, np.uint8)
    return v._lib.tsdf_sample(v._ctx, p.ctypes.data_as(C.c_void_p), 4, 12, 0, 0, mode, min_weight,
                              s.ctypes.data_as(_abi.FP), w.ctypes.data_as(_abi.FP),
                              g.ctypes.data_as(_abi.FP), ok.ctypes.data_as(_abi.U8P))


def raycast_call(v, mode, min_weight, step=0.025):
    o, d = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    depth, normal, hit = np.zeros(4, np.float32), np.zeros(12, np.float32), np.zeros(4, np.uint8)
    return v._lib.tsdf_raycast(v._ctx, o.ctypes.data_as(_abi.FP), d.ctypes.data_as(_abi.FP), 4, None,
                               0.0, 2.0, step, mode, min_weight, depth.ctypes.data_as(_abi.FP),
                               normal.ctypes.data_as(_abi.FP), hit.ctypes.data_as(_abi.U8P))


@pytest.mark.parametrize("what,doing,call", [("sample", "sampling", sample_call),
                                             ("raycast", "raycasting", raycast_call)])
def test_mode_and_weight_refusals(maps, shard, what, doing, call):
    g, _ = maps
    nan = float("nan")
    assert call(g, _abi.SAMPLE_NEAREST, 0.0) == _abi.TSDF_OK, text(g)
    refused(g, call(g, 7, 0.0), _abi.TSDF_EINVAL, MODE % what)
    refused(g, call(g, -1, nan), _abi.TSDF_EINVAL, MODE % what)  # the mode is checked first
    refused(g, call(g, _abi.SAMPLE_TRILINEAR, nan), _abi.TSDF_EINVAL, WEIGHT % what)
    refused(g, call(g, _abi.SAMPLE_NEAREST, -1.0), _abi.TSDF_EINVAL, WEIGHT % what)
    # the arguments are checked before the context's state
    refused(shard, call(shard, _abi.SAMPLE_NEAREST, 0.0), _abi.TSDF_EINVAL, SHARDED % (what, doing))
    refused(shard, call(shard, 7, 0.0), _abi.TSDF_EINVAL, MODE % what)
    refused(shard, call(shard, _abi.SAMPLE_NEAREST, nan), _abi.TSDF_EINVAL, WEIGHT % what)


def test_raycast_lattice_refusals_keep_their_place(maps, shard):
    """Raycast's own rules come after mode and min_weight and before the context's state."""
    g, _ = maps
    refused(g, raycast_call(g, _abi.SAMPLE_NEAREST, float("nan"), step=0.0), _abi.TSDF_EINVAL,
            WEIGHT % "raycast")
    refused(g, raycast_call(g, _abi.SAMPLE_NEAREST, 0.0, step=0.0), _abi.TSDF_EINVAL,
            "raycast: step must be positive")
    refused(shard, raycast_call(shard, _abi.SAMPLE_NEAREST, 0.0, step=float("inf")), _abi.TSDF_EINVAL,
            "raycast: t_min, t_max and step must be finite")


def test_border_pack_overflow_leaves_no_reduce_open():
    """Two contexts on one GPU share a brick; rank 1's pack into a buffer without room refuses,
    opens no reduce, and the reduce that follows gives the oracle's fields."""
    yaw0 = 0.3
    g = HipTSDFVolume.sharded(2, VS, TAU, device_ids=[0, 0], sector_yaw0=yaw0, **SMALL)
    o = [oracle.OracleTSDFVolume(VS, TAU, n_sectors=2, sector=r, sector_yaw0=yaw0) for r in range(2)]
    held = [[(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 0), (0, 0, 1), (-1, 0, 0)]]  # (0, 0, 0) twice
    for r in range(2):
        for v in (g[r], o[r]):
            v.import_bricks(*bricks(held[r], seed=r))
    dev = torch.device("cuda", 0)
    allk = torch.full((2, 3), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for r in range(2):
        assert g[r].brick_keys_into(allk[r].data_ptr(), 3) == 3
    send = torch.empty((1, 1028), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    counts, sent = np.array([3, 3], np.uint64), np.zeros(2, np.uint64)
    v = g[1]
    rc = v._lib.tsdf_border_pack_device(v._ctx, C.c_void_p(allk.data_ptr()),
                                        counts.ctypes.data_as(_abi.U64P), 3, 2, 1,
                                        C.c_void_p(send.data_ptr()), 0,
                                        sent.ctypes.data_as(_abi.U64P))
    refused(v, rc, _abi.TSDF_EOVERFLOW, "border pack needs 1 rows")
    assert sent.tolist() == [1, 0]
    assert v._lib.tsdf_import_bricks(v._ctx, None, None, None, 0) == _abi.TSDF_OK, text(v)
    assert border_reduce_local(g) == 1
    assert emulated_reduce_host(o) == [[0, 0], [1, 0]]
    for r in range(2):
        assert voxels_equal_bitwise(g[r].export_voxels(), o[r].export_voxels()), r
        g[r].close()
