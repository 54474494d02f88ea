"""Host-side mirror of the reference's mapping-backend interface over the C-ABI.

The reference selects a TSDF backend with the compile-time `MAP_BACKEND_IDX` of its (unshipped)
tsdf_map_node (README.md:44-50) and feeds it DLIO's deskewed world-frame cloud once per scan from a
subscriber callback (the slot is dliomapping.cpp:64-81).  Backend 3, VDBFusion, is the parity
target; its public API (PRBonn/vdbfusion `VDBVolume`: constructor (voxel_size, sdf_trunc,
space_carving), `integrate(points, extrinsic)` with extrinsic a (3,) origin or a (4,4) pose whose
translation is the origin, points already in the world frame) is what `TSDFVolume` mirrors, so a
user of that backend finds the same names, argument meanings and errors.

`semantics="voxblox"` selects backend idx 2's fusion rule instead (voxblox SimpleTsdfIntegrator
with a constant weight: projective distance, weight dropoff, clamps), and
`SimpleTsdfIntegrator` below mirrors voxblox's own names for it.

`TSDFVolume` is bound to one library exporting include/tsdf_hip.h; `HipTSDFVolume` is the product
class (MAP_BACKEND_IDX = 4) and loads libtsdf_hip.so only — it raises if the HIP library or the GPU
is missing, there is no CPU fallback.
"""
import ctypes as C
import math

import numpy as np

from . import _abi
from ._lib import load_hip_library


class TsdfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (_abi.STATUS_NAMES.get(code, str(code)), msg))
        self.code = code


def _origin_of(extrinsic):
    e = np.asarray(extrinsic, dtype=np.float64)
    if e.shape in ((3,), (3, 1)):
        return np.ascontiguousarray(e.reshape(3))
    if e.shape == (4, 4):
        return np.ascontiguousarray(e[:3, 3])
    if e.shape == (7,):
        return np.ascontiguousarray(e[:3])
    raise ValueError("origin/extrinsic must be a (3,) array, a (7,) pose or a (4,4) matrix")


def _quat_of(R):
    """(qx, qy, qz, qw) of a 3x3 rotation (Shepperd's method, float64)."""
    R = np.asarray(R, np.float64)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        return np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s,
                         0.25 * s])
    i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
    q = np.empty(4)
    q[i] = 0.25 * s
    q[j] = (R[j, i] + R[i, j]) / s
    q[k] = (R[k, i] + R[i, k]) / s
    q[3] = (R[k, j] - R[j, k]) / s
    return q


def _pose_of(extrinsic):
    """The (7,) pose (x, y, z, qx, qy, qz, qw) of a 4x4 extrinsic or a 7-vector; None for a bare
    (3,) origin."""
    e = np.asarray(extrinsic, dtype=np.float64)
    if e.shape == (7,):
        return np.ascontiguousarray(e)
    if e.shape == (4, 4):
        return np.ascontiguousarray(np.concatenate([e[:3, 3], _quat_of(e[:3, :3])]))
    return None


def _d3(a):
    return a.ctypes.data_as(_abi.D3)


class TSDFVolume:
    """A sparse TSDF volume of 8^3-voxel bricks behind the C-ABI of `lib`."""

    # where the library's "device" buffers live (the border-reduce entry points take pointers
    # into this memory): host memory for a CPU library, the context's GPU for libtsdf_hip.so
    tensor_device = "cpu"

    def __init__(self, lib, voxel_size, sdf_trunc, space_carving=False, **kw):
        self._lib = lib
        self._ctx = C.c_void_p()
        p = self.make_params(lib, voxel_size, sdf_trunc, space_carving, **kw)
        rc = lib.tsdf_create(C.byref(p), C.byref(self._ctx))
        if rc != _abi.TSDF_OK:
            self._ctx = C.c_void_p()
            raise TsdfError(rc, "tsdf_create failed (voxel_size=%g sdf_trunc=%g)" %
                            (voxel_size, sdf_trunc))
        self._adopt(p)

    def _adopt(self, p):
        self.params = p
        self.semantics = {v: k for k, v in _abi.SEMANTICS.items()}.get(p.semantics, "vdbfusion")
        self.voxel_size = float(p.voxel_size)
        self.sdf_trunc = float(p.sdf_trunc)
        self.space_carving = bool(p.space_carving)

    @staticmethod
    def make_params(lib, voxel_size, sdf_trunc, space_carving=False, min_range=0.0,
                    max_range=math.inf, max_bricks=1 << 20, max_points=1 << 18, device_id=0,
                    max_batch=32, pipeline=False, semantics="vdbfusion_f64", allow_clear=True,
                    use_weight_dropoff=True, max_weight=10000.0, n_sectors=0, sector=0,
                    sector_yaw0=0.0, max_bricks_hard=0, walk="two", use_const_weight=False,
                    method="simple", sector_input="fanout", sector_rule="index"):
        """tsdf_params from the VDBFusion / Voxblox-style keyword arguments."""
        if semantics not in _abi.SEMANTICS:
            raise ValueError("semantics must be one of %s" % sorted(_abi.SEMANTICS))
        p = _abi.default_params(lib)
        p.voxel_size = float(voxel_size)
        p.sdf_trunc = float(sdf_trunc)
        p.space_carving = 1 if space_carving else 0
        p.pipeline = int(pipeline) if not isinstance(pipeline, bool) else (1 if pipeline else 0)
        p.min_range = float(min_range)
        p.max_range = float(max_range)
        p.max_bricks = int(max_bricks)
        p.max_points = int(max_points)
        p.max_batch = int(max_batch)
        p.device_id = int(device_id)
        p.semantics = _abi.SEMANTICS[semantics]
        p.allow_clear = 1 if allow_clear else 0
        p.use_weight_dropoff = 1 if use_weight_dropoff else 0
        p.max_weight = float(max_weight)
        p.n_sectors = int(n_sectors)
        p.sector = int(sector)
        p.sector_yaw0 = float(sector_yaw0)
        p.max_bricks_hard = int(max_bricks_hard)
        # "two": k_count + k_place (default); "single": rays walked once (k_walk + k_spans) when the
        # band allows it
        p.walk = {"two": _abi.WALK_TWO, "single": _abi.WALK_SINGLE}[walk]
        # Voxblox getVoxelWeight: 1 (use_const_weight) or 1 / z^2 of the sensor-frame depth
        p.depth_weight = 0 if use_const_weight else 1
        # Voxblox's integrator (voxblox_ros `method`): "simple" or "merged" (ABI v8)
        if method not in _abi.VB_METHODS:
            raise ValueError("method must be one of %s" % sorted(_abi.VB_METHODS))
        p.voxblox_method = _abi.VB_METHODS[method]
        # tsdf_integrate_sectors' transfer (ABI v8): "fanout", "h2d" or "split"
        if sector_input not in _abi.SECTOR_INPUTS:
            raise ValueError("sector_input must be one of %s" % sorted(_abi.SECTOR_INPUTS))
        p.sector_input = _abi.SECTOR_INPUTS[sector_input]
        # which rays are sector k's (ABI v10): "index" (contiguous index ranges of each cloud,
        # DLIO's time order: sensor-frame column sectors; the default) or "world" (world-frame
        # pseudo-angle sectors)
        if sector_rule not in _abi.SECTOR_RULES:
            raise ValueError("sector_rule must be one of %s" % sorted(_abi.SECTOR_RULES))
        p.sector_rule = _abi.SECTOR_RULES[sector_rule]
        return p

    # -- lifecycle ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.tsdf_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != _abi.TSDF_OK:
            msg = self._lib.tsdf_last_error(self._ctx)
            raise TsdfError(rc, "%s: %s" % (what, msg.decode() if msg else ""))

    # -- integration ----------------------------------------------------------------------------
    def integrate(self, points, extrinsic):
        """VDBVolume.integrate: points (N,3) float32/float64 world-frame, extrinsic (3,) or (4,4)."""
        pts = np.asarray(points)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("points must be np.ndarray(n, 3)")
        if pts.dtype not in (np.float32, np.float64):
            raise TypeError("points dtype must be np.float32 or np.float64")
        pts = np.ascontiguousarray(pts)
        is64 = pts.dtype == np.float64
        step = 24 if is64 else 12
        pose = _pose_of(extrinsic)
        if pose is not None:  # the sensor's orientation too (Voxblox 1/z^2 weights)
            self._check(self._lib.tsdf_integrate_pose(self._ctx, pts.ctypes.data_as(C.c_void_p),
                                                      pts.shape[0], step, 0, 1 if is64 else 0,
                                                      _d3(pose)), "integrate_pose")
            return
        o = _origin_of(extrinsic)
        self._check(self._lib.tsdf_integrate(self._ctx, pts.ctypes.data_as(C.c_void_p),
                                             pts.shape[0], step, 0, 1 if is64 else 0, _d3(o)),
                    "integrate")

    def integrate_cloud(self, data, n, point_step, xyz_offset, origin, xyz_is_f64=False):
        """PointCloud2-style raw records (e.g. dlio::Point: point_step 32, x at offset 0)."""
        buf = np.frombuffer(data, dtype=np.uint8)
        if buf.size < n * point_step:
            raise ValueError("buffer smaller than n * point_step")
        pose = _pose_of(origin)
        if pose is not None:
            self._check(self._lib.tsdf_integrate_pose(self._ctx, buf.ctypes.data_as(C.c_void_p),
                                                      int(n), int(point_step), int(xyz_offset),
                                                      1 if xyz_is_f64 else 0, _d3(pose)),
                        "integrate_cloud")
            return
        o = _origin_of(origin)
        self._check(self._lib.tsdf_integrate(self._ctx, buf.ctypes.data_as(C.c_void_p), int(n),
                                             int(point_step), int(xyz_offset),
                                             1 if xyz_is_f64 else 0, _d3(o)), "integrate_cloud")

    def sync(self):
        self._check(self._lib.tsdf_sync(self._ctx), "sync")

    # -- read-out -------------------------------------------------------------------------------
    def query_dense(self, lo, hi):
        """(sdf, weight) of voxels lo..hi-1 as [z, y, x] float32 arrays."""
        lo = np.asarray(lo, np.int64).reshape(3)
        hi = np.asarray(hi, np.int64).reshape(3)
        dims = (hi - lo)
        if np.any(dims < 0):
            raise ValueError("hi < lo")
        s = np.empty((dims[2], dims[1], dims[0]), np.float32)
        w = np.empty_like(s)
        self._check(self._lib.tsdf_query_dense(self._ctx, lo.ctypes.data_as(_abi.L3),
                                               hi.ctypes.data_as(_abi.L3),
                                               s.ctypes.data_as(_abi.FP),
                                               w.ctypes.data_as(_abi.FP)), "query_dense")
        return s, w

    def _sample_fn(self, name):
        """An entry point of include/tsdf_hip_sample.h; a library without it (the feature is
        detected by the symbol) cannot sample, and says so."""
        fn = getattr(self._lib, name, None)
        if fn is None or fn.argtypes is None:
            raise NotImplementedError("%s does not export %s (sparse map queries and the raycast "
                                      "are part of libtsdf_hip.so only)" % (self._lib._name, name))
        return fn

    def sample(self, points, mode="trilinear", min_weight=0.0):
        """The field at world points (N, 3) float32 / float64 (float64 is rounded to float32):
        (sdf (N,), weight (N,), grad (N, 3), valid (N,) bool).  mode "nearest": the voxel holding
        the point, grad 0.  mode "trilinear": the interpolant of the 8 voxel centres around it and
        its analytic gradient (metres per metre), valid where all 8 are observed with weight >=
        min_weight; elsewhere (background, 0, 0).  include/tsdf_hip_sample.h states the arithmetic."""
        if mode not in _abi.SAMPLE_MODES:
            raise ValueError("mode must be one of %s" % sorted(_abi.SAMPLE_MODES))
        fn = self._sample_fn("tsdf_sample")
        pts = np.asarray(points)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("points must be np.ndarray(n, 3)")
        if pts.dtype not in (np.float32, np.float64):
            raise TypeError("points dtype must be np.float32 or np.float64")
        pts = np.ascontiguousarray(pts)
        is64 = pts.dtype == np.float64
        n = pts.shape[0]
        s = np.empty(n, np.float32)
        w = np.empty(n, np.float32)
        g = np.empty((n, 3), np.float32)
        v = np.empty(n, np.uint8)
        self._check(fn(self._ctx, pts.ctypes.data_as(C.c_void_p), n, 24 if is64 else 12, 0,
                       1 if is64 else 0, _abi.SAMPLE_MODES[mode], float(min_weight),
                       s.ctypes.data_as(_abi.FP), w.ctypes.data_as(_abi.FP),
                       g.ctypes.data_as(_abi.FP), v.ctypes.data_as(C.POINTER(C.c_uint8))), "sample")
        return s, w, g, v.astype(bool)

    def sample_cloud(self, data, n, point_step, xyz_offset, mode="trilinear", min_weight=0.0,
                     xyz_is_f64=False):
        """`sample` on PointCloud2-style raw records (e.g. dlio::Point, point_step 32)."""
        fn = self._sample_fn("tsdf_sample")
        buf = np.frombuffer(data, dtype=np.uint8)
        if buf.size < n * point_step:
            raise ValueError("buffer smaller than n * point_step")
        n = int(n)
        s = np.empty(n, np.float32)
        w = np.empty(n, np.float32)
        g = np.empty((n, 3), np.float32)
        v = np.empty(n, np.uint8)
        self._check(fn(self._ctx, buf.ctypes.data_as(C.c_void_p), n, int(point_step),
                       int(xyz_offset), 1 if xyz_is_f64 else 0, _abi.SAMPLE_MODES[mode],
                       float(min_weight), s.ctypes.data_as(_abi.FP), w.ctypes.data_as(_abi.FP),
                       g.ctypes.data_as(_abi.FP), v.ctypes.data_as(C.POINTER(C.c_uint8))),
                    "sample_cloud")
        return s, w, g, v.astype(bool)

    def _raycast_args(self, pose, t_min, t_max, step, mode):
        """(pose pointer or None, its array, t_min, t_max, step, mode code) of a raycast call."""
        if mode not in _abi.SAMPLE_MODES:
            raise ValueError("mode must be one of %s" % sorted(_abi.SAMPLE_MODES))
        T = None
        if pose is not None:
            T = np.asarray(pose, np.float64)
            if T.shape == (4, 4):
                T = T[:3]
            if T.shape != (3, 4):
                raise ValueError("pose must be a (3, 4) or (4, 4) matrix")
            T = np.ascontiguousarray(T)
        step = self.voxel_size / 2 if step is None else step
        return (None if T is None else _d3(T)), T, float(t_min), float(t_max), float(step), \
            _abi.SAMPLE_MODES[mode]

    def raycast(self, origins, dirs, pose=None, t_min=0.0, t_max=100.0, step=None, mode="nearest",
                min_weight=0.0, normals=True):
        """What the map shows along rays: (depth (N,), normal (N, 3) or None, hit (N,) bool).
        origins: (N, 3), or (3,) for one origin shared by every ray; dirs: (N, 3), not normalised
        by the call (depth counts in units of |dir|: unit directions give metres).  pose (3x4 or
        4x4, world from the rays' frame) transforms both; None takes the rays as given.  The ray
        is sampled every `step` (default voxel_size / 2) from t_min to t_max as `sample` samples
        points, and hits at the first front-facing zero crossing between two valid samples; depth
        is 0 and the normal (0, 0, 0) where there is none.  mode "trilinear" needs all eight
        voxels around a sample observed, which a sparse map seldom offers: "nearest" is the
        default.  include/tsdf_hip_raycast.h states the arithmetic."""
        fn = self._sample_fn("tsdf_raycast")
        pp, keep, t_min, t_max, step, code = self._raycast_args(pose, t_min, t_max, step, mode)
        d = np.asarray(dirs, np.float32)
        if d.ndim != 2 or d.shape[1] != 3:
            raise ValueError("dirs must be np.ndarray(n, 3)")
        o = np.asarray(origins, np.float32)
        if o.shape == (3,):
            o = np.broadcast_to(o, d.shape)
        if o.shape != d.shape:
            raise ValueError("origins must be (3,) or match dirs")
        o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
        n = d.shape[0]
        depth = np.empty(n, np.float32)
        normal = np.empty((n, 3), np.float32) if normals else None
        hit = np.empty(n, np.uint8)
        self._check(fn(self._ctx, o.ctypes.data_as(_abi.FP), d.ctypes.data_as(_abi.FP), n, pp,
                       t_min, t_max, step, code, float(min_weight), depth.ctypes.data_as(_abi.FP),
                       normal.ctypes.data_as(_abi.FP) if normals else None,
                       hit.ctypes.data_as(_abi.U8P)), "raycast")
        del keep
        return depth, normal, hit.astype(bool)

    # -- distance field of a box (include/tsdf_hip_esdf.h) ---------------------------------------
    def _esdf_fn(self, name):
        """An entry point of include/tsdf_hip_esdf.h, detected by the symbol like `_sample_fn`."""
        fn = getattr(self._lib, name, None)
        if fn is None or fn.argtypes is None:
            raise NotImplementedError("%s does not export %s (the distance field is part of "
                                      "libtsdf_hip.so only)" % (self._lib._name, name))
        return fn

    def esdf_radius(self, max_dist):
        """radius_vox of a distance field exact up to max_dist metres: ceil(max_dist / voxel_size)
        in double; ValueError outside 1..128 voxels."""
        r = math.ceil(float(max_dist) / float(self.voxel_size)) if math.isfinite(max_dist) else 0
        if not 1 <= r <= _abi.ESDF_MAX_RADIUS:
            raise ValueError("max_dist must span 1..%d voxels (voxel_size %g)"
                             % (_abi.ESDF_MAX_RADIUS, self.voxel_size))
        return int(r)

    def _esdf_args(self, lo, hi, max_dist, site_band):
        lo = np.ascontiguousarray(np.asarray(lo, np.int64).reshape(3))
        hi = np.ascontiguousarray(np.asarray(hi, np.int64).reshape(3))
        if np.any(hi < lo):
            raise ValueError("hi < lo")
        band = self.voxel_size if site_band is None else site_band
        return lo, hi, self.esdf_radius(max_dist), float(band)

    def esdf(self, lo, hi, max_dist, site_band=None, min_weight=0.0):
        """The Euclidean distance field of voxels lo..hi-1: (dist, flags) as [z, y, x] float32 /
        uint8 arrays.  dist is the distance in metres from the voxel's centre to the centre of the
        nearest surface voxel (a "site": observed with |sdf| <= site_band, default one voxel) of
        the box, exact up to max_dist and capped there, negative where the voxel is observed
        behind the surface.  flags: ESDF_OBSERVED | ESDF_SITE | ESDF_CAPPED of tsdf_map._abi.
        Only sites inside the box count: pad the box by the radius (`esdf.esdf_around` does) for
        clearances that are exact at its rim.  include/tsdf_hip_esdf.h states the rules."""
        lo, hi, radius, band = self._esdf_args(lo, hi, max_dist, site_band)
        fn = self._esdf_fn("tsdf_esdf_dense")
        dims = hi - lo
        dist = np.empty((dims[2], dims[1], dims[0]), np.float32)
        flags = np.empty(dist.shape, np.uint8)
        self._check(fn(self._ctx, lo.ctypes.data_as(_abi.L3), hi.ctypes.data_as(_abi.L3), radius,
                       band, float(min_weight), dist.ctypes.data_as(_abi.FP),
                       flags.ctypes.data_as(_abi.U8P)), "esdf")
        return dist, flags

    # -- column maps of a box (include/tsdf_hip_columns.h) ----------------------------------------
    def _columns_fn(self, name):
        """An entry point of include/tsdf_hip_columns.h, detected by the symbol like `_sample_fn`."""
        fn = getattr(self._lib, name, None)
        if fn is None or fn.argtypes is None:
            raise NotImplementedError("%s does not export %s (the column maps are part of "
                                      "libtsdf_hip.so only)" % (self._lib._name, name))
        return fn

    @staticmethod
    def _columns_args(lo, hi, min_occ, min_free):
        lo = np.ascontiguousarray(np.asarray(lo, np.int64).reshape(3))
        hi = np.ascontiguousarray(np.asarray(hi, np.int64).reshape(3))
        if np.any(hi < lo):
            raise ValueError("hi < lo")
        for name, v in (("min_occ", min_occ), ("min_free", min_free)):
            if not 1 <= int(v) <= 65535:
                raise ValueError("%s must be in 1..65535" % name)
        return lo, hi, int(min_occ), int(min_free)

    def column_map(self, lo, hi, occ_band=0.0, min_weight=0.0, min_occ=1, min_free=1):
        """The column maps of voxels lo..hi-1 as a `gridmap.ColumnMap` of [y, x] arrays: elev (the
        height in metres of the highest surface facing +z, NaN where the column has none), ceil
        (the lowest surface facing -z), n_occ / n_free (the observed voxels with sdf <= occ_band /
        above it), flags (COLUMN_* of tsdf_map._abi).  A voxel is observed when W > 0 and
        W >= min_weight; a column is OCCUPIED with n_occ >= min_occ, else FREE with
        n_free >= min_free, else unknown.  include/tsdf_hip_columns.h states the rules."""
        from .gridmap import ColumnMap
        lo, hi, min_occ, min_free = self._columns_args(lo, hi, min_occ, min_free)
        fn = self._columns_fn("tsdf_column_map")
        shape = (int(hi[1] - lo[1]), int(hi[0] - lo[0]))
        elev, ceil = np.empty(shape, np.float32), np.empty(shape, np.float32)
        n_occ, n_free = np.empty(shape, np.uint16), np.empty(shape, np.uint16)
        flags = np.empty(shape, np.uint8)
        self._check(fn(self._ctx, lo.ctypes.data_as(_abi.L3), hi.ctypes.data_as(_abi.L3),
                       float(occ_band), float(min_weight), min_occ, min_free,
                       elev.ctypes.data_as(_abi.FP), ceil.ctypes.data_as(_abi.FP),
                       n_occ.ctypes.data_as(_abi.U16P), n_free.ctypes.data_as(_abi.U16P),
                       flags.ctypes.data_as(_abi.U8P)), "column_map")
        return ColumnMap(elev, ceil, n_occ, n_free, flags, lo, hi, self.voxel_size)

    # -- frontier voxels (include/tsdf_hip_frontier.h) --------------------------------------------
    def _frontier_fn(self, name):
        """An entry point of include/tsdf_hip_frontier.h, detected by the symbol like `_sample_fn`."""
        fn = getattr(self._lib, name, None)
        if fn is None or fn.argtypes is None:
            raise NotImplementedError("%s does not export %s (the frontier voxels are part of "
                                      "libtsdf_hip.so only)" % (self._lib._name, name))
        return fn

    def _frontier_args(self, free_band, min_weight, connectivity, min_unknown):
        if int(connectivity) not in _abi.FRONTIER_CONNECTIVITIES:
            raise ValueError("connectivity must be 6, 18 or 26")
        if not 1 <= int(min_unknown) <= int(connectivity):
            raise ValueError("min_unknown must be in 1..connectivity")
        band = self.voxel_size if free_band is None else free_band
        return float(band), float(min_weight), int(connectivity), int(min_unknown)

    def frontier_counts(self, lo=None, hi=None, free_band=None, min_weight=0.0, connectivity=6,
                        min_unknown=1):
        """tsdf_frontier_count: {"n_bricks", "n_frontier_bricks", "n_voxels", "n_free"} of the set
        that `frontiers` would return; n_free is the explored free volume of the box in voxels."""
        fn = self._frontier_fn("tsdf_frontier_count")
        args = self._frontier_args(free_band, min_weight, connectivity, min_unknown)
        lo, hi, plo, phi = self._mesh_box(lo, hi)
        st = _abi.FrontierCounts()
        self._check(fn(self._ctx, plo, phi, *args, C.byref(st)), "frontier_counts")
        return st.as_dict()

    def frontiers(self, lo=None, hi=None, free_band=None, min_weight=0.0, connectivity=6,
                  min_unknown=1):
        """The frontier voxels of the voxel box [lo, hi) (the whole map without one) as a
        `frontier.FrontierSet`: the observed voxels (W > 0, W >= min_weight) with
        sdf >= free_band (default: one voxel size) that have at least `min_unknown` unobserved
        voxels among their 6, 18 or 26 neighbours.  Ordered by brick (z, y, x), then by in-brick
        voxel.  Meaningful on maps integrated with space carving; without it the set is the rim
        of the observed band.  include/tsdf_hip_frontier.h states the rules."""
        from .frontier import FrontierSet
        fn = self._frontier_fn("tsdf_frontier_voxels")
        args = self._frontier_args(free_band, min_weight, connectivity, min_unknown)
        lo, hi, plo, phi = self._mesh_box(lo, hi)
        st = _abi.FrontierCounts()
        for _ in range(2):
            n = self.frontier_counts(lo, hi, *args)["n_voxels"]
            coords = np.empty((n, 3), np.int32)
            nu = np.empty(n, np.uint8)
            d = np.empty((n, 3), np.int8)
            rc = fn(self._ctx, plo, phi, *args, coords.ctypes.data_as(_abi.I3),
                    nu.ctypes.data_as(_abi.U8P), d.ctypes.data_as(_abi.I8P), n, C.byref(st))
            if rc == _abi.TSDF_EOVERFLOW:
                continue
            self._check(rc, "frontiers")
            k = st.n_voxels
            return FrontierSet(coords[:k], nu[:k], d[:k], st.as_dict(), self.voxel_size)
        raise TsdfError(_abi.TSDF_EOVERFLOW, "frontiers: the map kept changing")

    def extract_triangle_mesh(self, fill_holes=True, min_weight=0.0, table="generated",
                              halo=None):
        """VDBVolume.extract_triangle_mesh: (vertices (3T, 3) float32, triangles (T, 3) int64) —
        marching cubes over every cube of 8 observed voxels (W > 0, W >= min_weight), as a soup
        (each triangle owns its 3 vertices).  fill_holes is accepted for API compatibility; cubes
        with an unobserved voxel are never meshed.  table: "generated" (face-consistent, the
        default) or "lorensen" (the published Lorensen / Bourke table, VDBFusion's).
        halo: (d_tiles_ptr, n_tiles) of neighbour bricks another rank owns (tsdf_extract_mesh_halo,
        in `tensor_device` memory): after a border reduce each rank meshes its own cubes.
        `extract_indexed_mesh` returns the same triangles with shared vertices and normals."""
        tab = _abi.MC_TABLES[table]
        n = C.c_uint64()

        def call(out, cap):
            if halo is None:
                return self._lib.tsdf_extract_mesh_table(self._ctx, float(min_weight), tab, out,
                                                         cap, C.byref(n))
            return self._lib.tsdf_extract_mesh_halo(self._ctx, float(min_weight), tab,
                                                    C.c_void_p(int(halo[0])), int(halo[1]), out,
                                                    cap, C.byref(n))

        self._check(call(None, 0), "extract_mesh")
        t = np.empty((n.value, 9), np.float32)
        if n.value:
            self._check(call(t.ctypes.data_as(_abi.FP), n.value), "extract_mesh")
        return t.reshape(-1, 3), np.arange(3 * t.shape[0], dtype=np.int64).reshape(-1, 3)

    # -- indexed mesh (include/tsdf_hip_mesh.h) --------------------------------------------------
    def _mesh_fn(self, name):
        """An entry point of include/tsdf_hip_mesh.h, detected by the symbol like `_sample_fn`."""
        fn = getattr(self._lib, name, None)
        if fn is None or fn.argtypes is None:
            raise NotImplementedError("%s does not export %s (the indexed mesh is part of "
                                      "libtsdf_hip.so only)" % (self._lib._name, name))
        return fn

    @staticmethod
    def _mesh_box(lo, hi):
        """(lo, hi) as int64[3] arrays with their ctypes pointers, or Nones for the whole map."""
        if lo is None and hi is None:
            return None, None, None, None
        if lo is None or hi is None:
            raise ValueError("lo and hi must both be given or both be None")
        lo = np.ascontiguousarray(np.asarray(lo, np.int64).reshape(3))
        hi = np.ascontiguousarray(np.asarray(hi, np.int64).reshape(3))
        return lo, hi, lo.ctypes.data_as(_abi.L3), hi.ctypes.data_as(_abi.L3)

    def indexed_mesh_counts(self, min_weight=0.0, table="generated", lo=None, hi=None):
        """tsdf_mesh_indexed_count: {"n_bricks", "n_vertices", "n_triangles"} of the mesh that
        `extract_indexed_mesh` would return."""
        fn = self._mesh_fn("tsdf_mesh_indexed_count")
        lo, hi, plo, phi = self._mesh_box(lo, hi)
        st = _abi.MeshCounts()
        self._check(fn(self._ctx, float(min_weight), _abi.MC_TABLES[table], plo, phi,
                       C.byref(st)), "indexed_mesh_counts")
        return st.as_dict()

    def extract_indexed_mesh(self, min_weight=0.0, table="generated", lo=None, hi=None,
                             normals=True):
        """The marching-cubes mesh with shared vertices: (vertices (V, 3) float32, triangles
        (T, 3) uint32, normals (V, 3) float32 or None).  One vertex per grid edge the surface
        crosses; `vertices[triangles]` is `extract_triangle_mesh`'s soup bit for bit, in its
        order.  Normals are the field's gradient at the vertex, unit length, pointing out of the
        surface.  lo / hi: mesh only the cubes whose min voxel lies in the voxel box [lo, hi)
        (`mesh.mesh_tiles` walks a map in such boxes).  include/tsdf_hip_mesh.h states the rules."""
        fn = self._mesh_fn("tsdf_mesh_indexed")
        tab = _abi.MC_TABLES[table]
        lo, hi, plo, phi = self._mesh_box(lo, hi)
        st = _abi.MeshCounts()
        for _ in range(2):
            n = self.indexed_mesh_counts(min_weight, table, lo, hi)
            v = np.empty((n["n_vertices"], 3), np.float32)
            t = np.empty((n["n_triangles"], 3), np.uint32)
            nr = np.empty_like(v) if normals else None
            rc = fn(self._ctx, float(min_weight), tab, plo, phi, v.ctypes.data_as(_abi.FP),
                    nr.ctypes.data_as(_abi.FP) if normals else None,
                    t.ctypes.data_as(_abi.U32P), v.shape[0], t.shape[0], C.byref(st))
            if rc == _abi.TSDF_EOVERFLOW:
                continue
            self._check(rc, "extract_indexed_mesh")
            nv, nt = st.n_vertices, st.n_triangles
            return v[:nv], t[:nt], (nr[:nv] if normals else None)
        raise TsdfError(_abi.TSDF_EOVERFLOW, "extract_indexed_mesh: the mesh kept changing")

    def num_bricks(self):
        n = C.c_uint64()
        self._check(self._lib.tsdf_num_bricks(self._ctx, C.byref(n)), "num_bricks")
        return n.value

    def export_bricks(self):
        """(coords (nb,3) int32, sdf (nb,8,8,8) [z,y,x], weight) sorted by brick (z, y, x)."""
        for _ in range(2):
            nb = self.num_bricks()
            coords = np.empty((nb, 3), np.int32)
            s = np.empty((nb, 8, 8, 8), np.float32)
            w = np.empty_like(s)
            n_out = C.c_uint64()
            rc = self._lib.tsdf_export_bricks(self._ctx, coords.ctypes.data_as(_abi.I3),
                                              s.ctypes.data_as(_abi.FP), w.ctypes.data_as(_abi.FP),
                                              nb, C.byref(n_out))
            if rc == _abi.TSDF_EOVERFLOW:
                continue
            self._check(rc, "export_bricks")
            k = n_out.value
            return coords[:k], s[:k], w[:k]
        raise TsdfError(_abi.TSDF_EOVERFLOW, "export_bricks: brick count kept changing")

    def brick_coords(self):
        """The map's brick coordinates (nb, 3) int32 in (z, y, x) order, without the voxels."""
        for _ in range(2):
            nb = self.num_bricks()
            coords = np.empty((nb, 3), np.int32)
            n_out = C.c_uint64()
            rc = self._lib.tsdf_export_bricks(self._ctx, coords.ctypes.data_as(_abi.I3), None,
                                              None, nb, C.byref(n_out))
            if rc == _abi.TSDF_EOVERFLOW:
                continue
            self._check(rc, "brick_coords")
            return coords[:n_out.value]
        raise TsdfError(_abi.TSDF_EOVERFLOW, "brick_coords: brick count kept changing")

    def import_bricks(self, coords, sdf, weight):
        coords = np.ascontiguousarray(coords, np.int32).reshape(-1, 3)
        sdf = np.ascontiguousarray(sdf, np.float32).reshape(-1, 512)
        weight = np.ascontiguousarray(weight, np.float32).reshape(-1, 512)
        if not (coords.shape[0] == sdf.shape[0] == weight.shape[0]):
            raise ValueError("coords/sdf/weight brick counts differ")
        self._check(self._lib.tsdf_import_bricks(self._ctx, coords.ctypes.data_as(_abi.I3),
                                                 sdf.ctypes.data_as(_abi.FP),
                                                 weight.ctypes.data_as(_abi.FP),
                                                 coords.shape[0]), "import_bricks")

    def export_voxels(self):
        """Every voxel with weight > 0: (ijk (n,3) int32, sdf (n,), weight (n,)), sorted (z,y,x)."""
        return bricks_to_voxels(*self.export_bricks())

    # -- removing bricks (include/tsdf_hip_prune.h) ---------------------------------------------
    def _prune_fn(self, name):
        """An entry point of include/tsdf_hip_prune.h, detected by the symbol like `_sample_fn`."""
        fn = getattr(self._lib, name, None)
        if fn is None or fn.argtypes is None:
            raise NotImplementedError("%s does not export %s (prune and evict are part of "
                                      "libtsdf_hip.so only)" % (self._lib._name, name))
        return fn

    @staticmethod
    def _box(lo, hi):
        lo = np.ascontiguousarray(np.asarray(lo, np.int64).reshape(3))
        hi = np.ascontiguousarray(np.asarray(hi, np.int64).reshape(3))
        if np.any(lo > hi):
            raise ValueError("lo > hi")
        # (bricks beyond the packable range do not exist: clamping changes no answer)
        lo = np.clip(lo, _abi.BRICK_COORD_MIN, _abi.BRICK_COORD_MAX).astype(np.int32)
        hi = np.clip(hi, _abi.BRICK_COORD_MIN, _abi.BRICK_COORD_MAX).astype(np.int32)
        return lo, hi

    def prune(self, min_weight):
        """VDBVolume.prune: every voxel with weight < min_weight goes back to the background, and
        every brick left without an observed voxel is removed, in place.  Returns the number of
        bricks removed."""
        fn = self._prune_fn("tsdf_prune")
        n = C.c_uint64()
        self._check(fn(self._ctx, float(min_weight), C.byref(n)), "prune")
        return n.value

    def count_outside(self, lo, hi):
        """The bricks whose brick coordinate (voxel // 8) is not in lo <= b < hi on every axis."""
        fn = self._prune_fn("tsdf_count_outside")
        lo, hi = self._box(lo, hi)
        n = C.c_uint64()
        self._check(fn(self._ctx, lo.ctypes.data_as(_abi.I3), hi.ctypes.data_as(_abi.I3),
                       C.byref(n)), "count_outside")
        return n.value

    def evict_outside(self, lo, hi, copy_out=True):
        """Remove the bricks outside the brick box lo <= b < hi.  copy_out: return them as
        `export_bricks` would, (coords, sdf, weight) sorted by brick (z, y, x) -- `import_bricks`
        takes them back; otherwise return their number."""
        fn = self._prune_fn("tsdf_evict_outside")
        blo, bhi = self._box(lo, hi)
        plo, phi = blo.ctypes.data_as(_abi.I3), bhi.ctypes.data_as(_abi.I3)
        n_out = C.c_uint64()
        if not copy_out:
            self._check(fn(self._ctx, plo, phi, None, None, None, 0, C.byref(n_out)),
                        "evict_outside")
            return n_out.value
        for _ in range(2):
            nb = self.count_outside(blo, bhi)
            coords = np.empty((nb, 3), np.int32)
            s = np.empty((nb, 8, 8, 8), np.float32)
            w = np.empty_like(s)
            rc = fn(self._ctx, plo, phi, coords.ctypes.data_as(_abi.I3),
                    s.ctypes.data_as(_abi.FP), w.ctypes.data_as(_abi.FP), nb, C.byref(n_out))
            if rc == _abi.TSDF_EOVERFLOW:
                continue
            self._check(rc, "evict_outside")
            k = n_out.value
            return coords[:k], s[:k], w[:k]
        raise TsdfError(_abi.TSDF_EOVERFLOW, "evict_outside: brick count kept changing")

    # -- merging another map into this one (include/tsdf_hip_merge.h) ----------------------------
    def _merge_fn(self, name):
        """An entry point of include/tsdf_hip_merge.h, detected by the symbol like `_sample_fn`."""
        fn = getattr(self._lib, name, None)
        if fn is None or fn.argtypes is None:
            raise NotImplementedError("%s does not export %s (merging maps under a transform is "
                                      "part of libtsdf_hip.so only)" % (self._lib._name, name))
        return fn

    def merge_from(self, src, pose, mode="trilinear", min_weight=0.0, dry_run=False):
        """Merge the map of `src` into this one at `pose` = T_dst_src ((3, 4) or (4, 4),
        x_dst = R x_src + t): `src` is resampled at this volume's voxel centres (mode "nearest" or
        "trilinear", valid where `sample` is) and fused by weight, on the GPU.  Resampling is not
        copying: the trilinear mode keeps only fully observed cubes.  dry_run: change nothing.
        Returns the counts of tsdf_merge_stats as a dict; on TsdfError (TSDF_ENOMEM: the new
        bricks do not fit and the pool cannot grow) both maps are as they were and the error's
        `stats` holds the counts.  include/tsdf_hip_merge.h states the rules."""
        if mode not in _abi.SAMPLE_MODES:
            raise ValueError("mode must be one of %s" % sorted(_abi.SAMPLE_MODES))
        fn = self._merge_fn("tsdf_merge_count" if dry_run else "tsdf_merge_transformed")
        if not isinstance(src, TSDFVolume):
            raise TypeError("src must be a TSDFVolume")
        if src._lib is not self._lib:
            raise ValueError("src belongs to another library")
        T = np.asarray(pose, np.float64)
        if T.shape == (4, 4):
            T = T[:3]
        if T.shape != (3, 4):
            raise ValueError("pose must be a (3, 4) or (4, 4) matrix")
        T = np.ascontiguousarray(T)
        st = _abi.MergeStats()
        rc = fn(self._ctx, src._ctx, _d3(T), _abi.SAMPLE_MODES[mode], float(min_weight),
                C.byref(st))
        try:
            self._check(rc, "merge_from")
        except TsdfError as e:
            e.stats = st.as_dict()
            raise
        return st.as_dict()

    # -- coarsening another map 2:1 into this one (include/tsdf_hip_coarsen.h) -------------------
    def _coarsen_fn(self, name):
        """An entry point of include/tsdf_hip_coarsen.h, detected by the symbol like `_sample_fn`."""
        fn = getattr(self._lib, name, None)
        if fn is None or fn.argtypes is None:
            raise NotImplementedError("%s does not export %s (coarsening a map is part of "
                                      "libtsdf_hip.so only)" % (self._lib._name, name))
        return fn

    def coarsen_from(self, src, min_children=1, min_weight=0.0, box=None, side="inside",
                     dry_run=False):
        """Fuse the 2:1 reduction of `src` (half this volume's voxel size) into this map, on the
        GPU: a coarse voxel is the weight-weighted mean of its valid children (W > 0 and
        W >= min_weight) when at least `min_children` of the eight are valid, with their mean
        weight.  box = (lo, hi): only the source bricks lo <= b < hi (side "inside") or all the
        others ("outside"), the predicate of `count_outside`.  dry_run: change nothing.
        Returns the counts of tsdf_coarsen_stats as a dict; on TsdfError (TSDF_ENOMEM: the new
        bricks do not fit and the pool cannot grow) both maps are as they were and the error's
        `stats` holds the counts.  include/tsdf_hip_coarsen.h states the rules."""
        if side not in _abi.COARSEN_SIDES:
            raise ValueError("side must be one of %s" % sorted(_abi.COARSEN_SIDES))
        fn = self._coarsen_fn("tsdf_coarsen_count" if dry_run else "tsdf_coarsen_into")
        if not isinstance(src, TSDFVolume):
            raise TypeError("src must be a TSDFVolume")
        if src._lib is not self._lib:
            raise ValueError("src belongs to another library")
        if not 1 <= int(min_children) <= 8:
            raise ValueError("min_children must be 1..8")
        plo = phi = None
        if box is not None:
            lo, hi = self._box(*box)
            plo, phi = lo.ctypes.data_as(_abi.I3), hi.ctypes.data_as(_abi.I3)
        st = _abi.CoarsenStats()
        rc = fn(self._ctx, src._ctx, plo, phi, _abi.COARSEN_SIDES[side], int(min_children),
                float(min_weight), C.byref(st))
        try:
            self._check(rc, "coarsen_from")
        except TsdfError as e:
            e.stats = st.as_dict()
            raise
        return st.as_dict()

    def save(self, path):
        """Checkpoint: the brick map as .npz (keys, sdf, weight, parameters)."""
        c, s, w = self.export_bricks()
        np.savez_compressed(path, coords=c, sdf=s, weight=w, voxel_size=self.voxel_size,
                            sdf_trunc=self.sdf_trunc, space_carving=self.space_carving)

    def load(self, path):
        """Resume from save(): merges the stored bricks into this volume."""
        with np.load(path, allow_pickle=False) as z:
            if not np.isclose(float(z["voxel_size"]), self.voxel_size):
                raise ValueError("checkpoint voxel_size differs")
            self.import_bricks(z["coords"], z["sdf"], z["weight"])

    # -- border-brick reduce (multi-GPU read-out; tsdf_map.distributed drives it) ---------------
    def brick_keys_into(self, d_keys_ptr, cap):
        """Write this volume's packed brick keys to `tensor_device` memory; returns the count."""
        n = C.c_uint64()
        self._check(self._lib.tsdf_brick_keys_device(self._ctx, C.c_void_p(int(d_keys_ptr)),
                                                     int(cap), C.byref(n)), "brick_keys")
        return n.value

    def border_pack(self, d_all_keys_ptr, counts, stride, world, rank, d_send_ptr, cap_rows):
        """Pack the bricks a lower rank owns (they keep their mass until border_commit); returns
        the rows per destination."""
        cnt = np.ascontiguousarray(counts, np.uint64)
        out = np.zeros(int(world), np.uint64)
        self._check(self._lib.tsdf_border_pack_device(
            self._ctx, C.c_void_p(int(d_all_keys_ptr)), cnt.ctypes.data_as(_abi.U64P),
            int(stride), int(world), int(rank), C.c_void_p(int(d_send_ptr)), int(cap_rows),
            out.ctypes.data_as(_abi.U64P)), "border_pack")
        return [int(x) for x in out]

    def border_merge(self, d_recv_ptr, recv_counts):
        cnt = np.ascontiguousarray(recv_counts, np.uint64)
        self._check(self._lib.tsdf_border_merge_device(
            self._ctx, C.c_void_p(int(d_recv_ptr)), cnt.ctypes.data_as(_abi.U64P), cnt.shape[0]),
            "border_merge")

    def border_commit(self, commit=True):
        """Close the border reduce: commit (every rank merged) resets the sent bricks, abort
        restores the merged ones; either way the context takes scans again."""
        self._check(self._lib.tsdf_border_commit_device(self._ctx, 1 if commit else 0),
                    "border_commit")

    def halo_keys_into(self, d_keys_ptr, cap):
        """The neighbour bricks this volume needs to mesh its own and does not observe
        (tsdf_halo_keys_device): returns the count; writes them when cap suffices."""
        n = C.c_uint64()
        rc = self._lib.tsdf_halo_keys_device(self._ctx, C.c_void_p(int(d_keys_ptr or 0)), int(cap),
                                             C.byref(n))
        if rc != _abi.TSDF_EOVERFLOW or cap:
            self._check(rc, "halo_keys")
        return n.value

    def halo_pack(self, d_req_ptr, n_req, d_send_ptr, cap_rows):
        """Tiles of the requested bricks this volume observes; returns the rows written."""
        n = C.c_uint64()
        self._check(self._lib.tsdf_halo_pack_device(self._ctx, C.c_void_p(int(d_req_ptr)),
                                                    int(n_req), C.c_void_p(int(d_send_ptr)),
                                                    int(cap_rows), C.byref(n)), "halo_pack")
        return n.value

    # -- stats ----------------------------------------------------------------------------------
    def stats(self):
        st = _abi.TsdfStats()
        self._check(self._lib.tsdf_get_stats(self._ctx, C.byref(st)), "get_stats")
        return st.as_dict()

    def reset_stats(self):
        self._check(self._lib.tsdf_reset_stats(self._ctx), "reset_stats")


def integrate_sectors(volumes, points, extrinsic):
    """tsdf_integrate_sectors: one host cloud for the sector-sharded contexts `volumes` (volume k
    created with n_sectors = len(volumes), sector = k, one per GPU; DESIGN.md §7, live N-GPU
    input).  A (7,) pose or (4,4) extrinsic carries the sensor orientation; a bare (3,) origin
    goes to tsdf_integrate_sectors_origin and, like `integrate`, carries none (Voxblox's constant
    weight), so the sharded field equals the unsharded one for every semantics."""
    pts = np.ascontiguousarray(points)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.dtype not in (np.float32, np.float64):
        raise ValueError("points must be np.ndarray(n, 3) of float32 / float64")
    v0 = volumes[0]
    ctxs = (C.c_void_p * len(volumes))(*[v._ctx.value for v in volumes])
    is64 = pts.dtype == np.float64
    pose = _pose_of(extrinsic)
    if pose is None:
        fn, arg = v0._lib.tsdf_integrate_sectors_origin, _origin_of(extrinsic)
    else:
        fn, arg = v0._lib.tsdf_integrate_sectors, np.ascontiguousarray(pose, np.float64)
    rc = fn(ctxs, len(volumes), pts.ctypes.data_as(C.c_void_p), pts.shape[0], 24 if is64 else 12,
            0, 1 if is64 else 0, _d3(arg))
    v0._check(rc, "integrate_sectors")


def border_reduce_local(volumes):
    """tsdf_border_reduce_local: the border-brick reduce among sector volumes of this process
    (peer copies between their GPUs, no collective); returns the tiles merged."""
    v0 = volumes[0]
    ctxs = (C.c_void_p * len(volumes))(*[v._ctx.value for v in volumes])
    moved = C.c_uint64()
    v0._check(v0._lib.tsdf_border_reduce_local(ctxs, len(volumes), C.byref(moved)),
              "border_reduce_local")
    return moved.value


def integrate_sectors_cloud(volumes, data, n, point_step, xyz_offset, extrinsic, xyz_is_f64=False):
    """integrate_sectors on PointCloud2-style raw records (e.g. dlio::Point, point_step 32)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    if buf.size < n * point_step:
        raise ValueError("buffer smaller than n * point_step")
    v0 = volumes[0]
    ctxs = (C.c_void_p * len(volumes))(*[v._ctx.value for v in volumes])
    pose = _pose_of(extrinsic)
    if pose is None:
        fn, arg = v0._lib.tsdf_integrate_sectors_origin, _origin_of(extrinsic)
    else:
        fn, arg = v0._lib.tsdf_integrate_sectors, np.ascontiguousarray(pose, np.float64)
    v0._check(fn(ctxs, len(volumes), buf.ctypes.data_as(C.c_void_p), int(n), int(point_step),
                 int(xyz_offset), 1 if xyz_is_f64 else 0, _d3(arg)), "integrate_sectors_cloud")


def extract_mesh_local(volumes, min_weight=0.0, table="generated"):
    """tsdf_extract_mesh_local: the mesh of sector volumes of this process (border reduce, halo
    exchange, one mesh per volume); returns (vertices (3T, 3), triangles (T, 3)) with the volumes'
    soups in volume order, and the triangles per volume."""
    v0 = volumes[0]
    ctxs = (C.c_void_p * len(volumes))(*[v._ctx.value for v in volumes])
    tab = _abi.MC_TABLES[table]
    n = C.c_uint64()
    v0._check(v0._lib.tsdf_extract_mesh_local(ctxs, len(volumes), float(min_weight), tab, None, 0,
                                              C.byref(n)), "extract_mesh_local")
    t = np.empty((n.value, 9), np.float32)
    if n.value:
        v0._check(v0._lib.tsdf_extract_mesh_local(ctxs, len(volumes), float(min_weight), tab,
                                                  t.ctypes.data_as(_abi.FP), n.value, C.byref(n)),
                  "extract_mesh_local")
    return t.reshape(-1, 3), np.arange(3 * t.shape[0], dtype=np.int64).reshape(-1, 3)


def bricks_to_voxels(coords, sdf, weight):
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    s = np.asarray(sdf, np.float32).reshape(-1, 8, 8, 8)
    w = np.asarray(weight, np.float32).reshape(-1, 8, 8, 8)
    b, z, y, x = np.nonzero(w > 0)
    ijk = np.stack([coords[b, 0] * 8 + x, coords[b, 1] * 8 + y, coords[b, 2] * 8 + z], 1)
    order = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))
    return ijk[order].astype(np.int32), s[b, z, y, x][order], w[b, z, y, x][order]


class HipTSDFVolume(TSDFVolume):
    """MAP_BACKEND_IDX = 4: the MI355X backend (libtsdf_hip.so).  Adds the device-resident entry
    points; device arrays are anything exposing a HIP device pointer (e.g. torch tensors)."""

    def __init__(self, voxel_size, sdf_trunc, space_carving=False, **kw):
        super().__init__(load_hip_library(), voxel_size, sdf_trunc, space_carving, **kw)
        self.tensor_device = "cuda:%d" % self.params.device_id

    @classmethod
    def sharded(cls, n, voxel_size, sdf_trunc, device_ids=None, **kw):
        """tsdf_create_sharded: n volumes in this process, volume k on device_ids[k] (default k)
        as azimuth sector k of n.  Feed them with `integrate_sectors`, reduce their border bricks
        with `border_reduce_local`."""
        lib = load_hip_library()
        kw = {k: v for k, v in kw.items() if k not in ("n_sectors", "sector", "device_id")}
        p = cls.make_params(lib, voxel_size, sdf_trunc, **kw)
        ids = None if device_ids is None else (C.c_int32 * n)(*[int(d) for d in device_ids])
        out = (C.c_void_p * n)()
        rc = lib.tsdf_create_sharded(C.byref(p), int(n), ids, out)
        if rc != _abi.TSDF_OK:
            raise TsdfError(rc, "tsdf_create_sharded failed (n=%d)" % n)
        vols = []
        for k in range(n):
            v = cls.__new__(cls)
            v._lib = lib
            v._ctx = C.c_void_p(out[k])
            q = _abi.TsdfParams.from_buffer_copy(p)
            q.device_id = int(device_ids[k]) if device_ids is not None else k
            q.n_sectors = n if n > 1 else 0
            q.sector = k
            v._adopt(q)
            v.tensor_device = "cuda:%d" % q.device_id
            vols.append(v)
        return vols

    def empty_like(self):
        """A new, empty volume with this one's parameters (on the same device)."""
        out = type(self).__new__(type(self))
        out._lib = self._lib
        out._ctx = C.c_void_p()
        p = _abi.TsdfParams.from_buffer_copy(self.params)
        rc = self._lib.tsdf_create(C.byref(p), C.byref(out._ctx))
        if rc != _abi.TSDF_OK:
            out._ctx = C.c_void_p()
            raise TsdfError(rc, "tsdf_create failed (empty_like)")
        out._adopt(p)
        out.tensor_device = self.tensor_device
        return out

    def transformed(self, pose, **kw):
        """A new volume with this one's parameters, holding this map moved by `pose` (T_new_this):
        `merge_from(self, pose, **kw)` into an empty volume.  This volume is not changed."""
        self._merge_fn("tsdf_merge_transformed")
        out = self.empty_like()
        try:
            out.merge_from(self, pose, **kw)
        except Exception:
            out.close()
            raise
        return out

    def coarsened(self, min_children=1, min_weight=0.0, **kw):
        """A new volume with this one's parameters except `voxel_size` doubled, holding this map
        coarsened 2:1: `coarsen_from(self, min_children, min_weight, **kw)` into an empty volume
        (the truncation distance stays, as include/tsdf_hip_coarsen.h requires).  This volume is
        not changed."""
        self._coarsen_fn("tsdf_coarsen_into")
        out = type(self).__new__(type(self))
        out._lib = self._lib
        out._ctx = C.c_void_p()
        p = _abi.TsdfParams.from_buffer_copy(self.params)
        p.voxel_size = 2.0 * float(self.params.voxel_size)
        rc = self._lib.tsdf_create(C.byref(p), C.byref(out._ctx))
        if rc != _abi.TSDF_OK:
            out._ctx = C.c_void_p()
            raise TsdfError(rc, "tsdf_create failed (coarsened)")
        out._adopt(p)
        out.tensor_device = self.tensor_device
        try:
            out.coarsen_from(self, min_children, min_weight, **kw)
        except Exception:
            out.close()
            raise
        return out

    def integrate_device(self, d_xyz_ptr, n, extrinsic):
        o = _origin_of(extrinsic)
        self._check(self._lib.tsdf_integrate_device(self._ctx, C.c_void_p(int(d_xyz_ptr)), int(n),
                                                    _d3(o)), "integrate_device")

    def integrate_batch_device(self, d_xyz_ptr, scan_offsets, origins):
        """origins: (n, 3) ray origins, or (n, 7) poses (x, y, z, qx, qy, qz, qw)."""
        offs = np.ascontiguousarray(scan_offsets, np.uint64)
        a = np.asarray(origins, np.float64)
        fn, k = ((self._lib.tsdf_integrate_batch_device_pose, 7) if a.ndim == 2 and a.shape[1] == 7
                 else (self._lib.tsdf_integrate_batch_device, 3))
        org = np.ascontiguousarray(a).reshape(-1, k)
        if offs.shape[0] != org.shape[0] + 1:
            raise ValueError("scan_offsets must have n_scans + 1 entries")
        self._check(fn(self._ctx, C.c_void_p(int(d_xyz_ptr)), offs.ctypes.data_as(_abi.U64P),
                       org.shape[0], org.ctypes.data_as(_abi.D3)), "integrate_batch_device")

    def integrate_batch_device_pose(self, d_xyz_ptr, scan_offsets, poses):
        """integrate_batch_device with one (x, y, z, qx, qy, qz, qw) pose per scan, (n, 7)."""
        p = np.asarray(poses, np.float64)
        if p.ndim != 2 or p.shape[1] != 7:
            raise ValueError("poses must be (n_scans, 7)")
        self.integrate_batch_device(d_xyz_ptr, scan_offsets, p)

    def sample_device(self, d_xyz_ptr, n, d_sdf_ptr, d_weight_ptr, d_grad_ptr, d_valid_ptr,
                      mode="trilinear", min_weight=0.0):
        """`sample` for n device points (n x 3 float32) into caller-given device buffers: sdf and
        weight (n float32), grad (3 n float32, or None / 0 to skip it), valid (n uint8).  The
        points must be complete before the call; the outputs are complete when it returns."""
        if mode not in _abi.SAMPLE_MODES:
            raise ValueError("mode must be one of %s" % sorted(_abi.SAMPLE_MODES))
        fn = self._sample_fn("tsdf_sample_device")
        self._check(fn(self._ctx, C.c_void_p(int(d_xyz_ptr or 0)), int(n), _abi.SAMPLE_MODES[mode],
                       float(min_weight), C.c_void_p(int(d_sdf_ptr or 0)),
                       C.c_void_p(int(d_weight_ptr or 0)), C.c_void_p(int(d_grad_ptr or 0)),
                       C.c_void_p(int(d_valid_ptr or 0))), "sample_device")

    def raycast_device(self, d_org_ptr, d_dir_ptr, n, d_depth_ptr, d_normal_ptr, d_hit_ptr,
                       pose=None, t_min=0.0, t_max=100.0, step=None, mode="nearest",
                       min_weight=0.0):
        """`raycast` for n device rays (origins and directions, n x 3 float32 each) into
        caller-given device buffers: depth (n float32), normal (3 n float32, or None / 0 to skip
        it), hit (n uint8).  The rays must be complete before the call; the outputs are complete
        when it returns."""
        fn = self._sample_fn("tsdf_raycast_device")
        pp, keep, t_min, t_max, step, code = self._raycast_args(pose, t_min, t_max, step, mode)
        self._check(fn(self._ctx, C.c_void_p(int(d_org_ptr or 0)), C.c_void_p(int(d_dir_ptr or 0)),
                       int(n), pp, t_min, t_max, step, code, float(min_weight),
                       C.c_void_p(int(d_depth_ptr or 0)), C.c_void_p(int(d_normal_ptr or 0)),
                       C.c_void_p(int(d_hit_ptr or 0))), "raycast_device")
        del keep

    def esdf_device(self, lo, hi, max_dist, site_band=None, min_weight=0.0, flags=True):
        """`esdf` into device tensors on the volume's GPU: (dist [z, y, x] float32, flags [z, y, x]
        uint8, or None with flags=False), complete when the call returns."""
        import torch
        lo, hi, radius, band = self._esdf_args(lo, hi, max_dist, site_band)
        fn = self._esdf_fn("tsdf_esdf_dense_device")
        shape = tuple(int(d) for d in (hi - lo)[::-1])
        dist = torch.empty(shape, dtype=torch.float32, device=self.tensor_device)
        fl = torch.empty(shape, dtype=torch.uint8, device=self.tensor_device) if flags else None
        torch.cuda.synchronize(dist.device)
        self._check(fn(self._ctx, lo.ctypes.data_as(_abi.L3), hi.ctypes.data_as(_abi.L3), radius,
                       band, float(min_weight), C.c_void_p(dist.data_ptr()),
                       C.c_void_p(fl.data_ptr() if flags else 0)), "esdf_device")
        return dist, fl

    def column_map_device(self, lo, hi, occ_band=0.0, min_weight=0.0, min_occ=1, min_free=1):
        """`column_map` into device tensors on the volume's GPU: (elev, ceil float32, n_occ, n_free
        uint16, flags uint8), each [y, x], complete when the call returns."""
        import torch
        lo, hi, min_occ, min_free = self._columns_args(lo, hi, min_occ, min_free)
        fn = self._columns_fn("tsdf_column_map_device")
        shape = (int(hi[1] - lo[1]), int(hi[0] - lo[0]))
        out = [torch.empty(shape, dtype=dt, device=self.tensor_device)
               for dt in (torch.float32, torch.float32, torch.uint16, torch.uint16, torch.uint8)]
        torch.cuda.synchronize(out[0].device)
        self._check(fn(self._ctx, lo.ctypes.data_as(_abi.L3), hi.ctypes.data_as(_abi.L3),
                       float(occ_band), float(min_weight), min_occ, min_free,
                       *[C.c_void_p(t.data_ptr()) for t in out]), "column_map_device")
        return tuple(out)

    def frontiers_device(self, lo=None, hi=None, free_band=None, min_weight=0.0, connectivity=6,
                         min_unknown=1):
        """`frontiers` into device tensors on the volume's GPU: (coords (N, 3) int32, n_unknown
        (N,) uint8, dir (N, 3) int8, counts dict), complete when the call returns."""
        import torch
        fn = self._frontier_fn("tsdf_frontier_voxels_device")
        args = self._frontier_args(free_band, min_weight, connectivity, min_unknown)
        lo, hi, plo, phi = self._mesh_box(lo, hi)
        st = _abi.FrontierCounts()
        for _ in range(2):
            n = self.frontier_counts(lo, hi, *args)["n_voxels"]
            coords = torch.empty((n, 3), dtype=torch.int32, device=self.tensor_device)
            nu = torch.empty((n,), dtype=torch.uint8, device=self.tensor_device)
            d = torch.empty((n, 3), dtype=torch.int8, device=self.tensor_device)
            torch.cuda.synchronize(coords.device)
            rc = fn(self._ctx, plo, phi, *args, C.c_void_p(coords.data_ptr()),
                    C.c_void_p(nu.data_ptr()), C.c_void_p(d.data_ptr()), n, C.byref(st))
            if rc == _abi.TSDF_EOVERFLOW:
                continue
            self._check(rc, "frontiers_device")
            k = st.n_voxels
            return coords[:k], nu[:k], d[:k], st.as_dict()
        raise TsdfError(_abi.TSDF_EOVERFLOW, "frontiers_device: the map kept changing")

    def indexed_mesh_device(self, min_weight=0.0, table="generated", lo=None, hi=None,
                            normals=True):
        """`extract_indexed_mesh` into device tensors on the volume's GPU: (vertices (V, 3)
        float32, triangles (T, 3) uint32, normals (V, 3) float32 or None), complete when the call
        returns."""
        import torch
        fn = self._mesh_fn("tsdf_mesh_indexed_device")
        tab = _abi.MC_TABLES[table]
        lo, hi, plo, phi = self._mesh_box(lo, hi)
        st = _abi.MeshCounts()
        for _ in range(2):
            n = self.indexed_mesh_counts(min_weight, table, lo, hi)
            nv, nt = n["n_vertices"], n["n_triangles"]
            v = torch.empty((nv, 3), dtype=torch.float32, device=self.tensor_device)
            t = torch.empty((nt, 3), dtype=torch.uint32, device=self.tensor_device)
            nr = torch.empty_like(v) if normals else None
            torch.cuda.synchronize(v.device)
            rc = fn(self._ctx, float(min_weight), tab, plo, phi, C.c_void_p(v.data_ptr()),
                    C.c_void_p(nr.data_ptr() if normals else 0), C.c_void_p(t.data_ptr()), nv, nt,
                    C.byref(st))
            if rc == _abi.TSDF_EOVERFLOW:
                continue
            self._check(rc, "indexed_mesh_device")
            nv, nt = st.n_vertices, st.n_triangles
            return v[:nv], t[:nt], (nr[:nv] if normals else None)
        raise TsdfError(_abi.TSDF_EOVERFLOW, "indexed_mesh_device: the mesh kept changing")

    def align_terms(self, points, pose, min_weight=0.0, n=None):
        """Gauss-Newton terms of the point-to-TSDF error of a cloud under `pose` (3x4 or 4x4, world
        from cloud): (H (6, 6), b (6,), e = sum r^2, n_valid) over the points whose trilinear sample
        is valid, r the sampled distance and J = [g, q x g] for a left perturbation (dt, dtheta).
        points: an (N, 3) array (copied to the device), or a device pointer with n points of
        float32 xyz.  The same inputs give the same bits on every call."""
        fn = self._sample_fn("tsdf_align_terms_device")
        T = np.asarray(pose, np.float64)
        if T.shape == (4, 4):
            T = T[:3]
        if T.shape != (3, 4):
            raise ValueError("pose must be a (3, 4) or (4, 4) matrix")
        T = np.ascontiguousarray(T)
        keep = None
        if isinstance(points, (int, np.integer)):
            if n is None:
                raise ValueError("a device pointer needs n")
            ptr = int(points)
        else:
            import torch
            pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
            keep = torch.from_numpy(pts).to(self.tensor_device)
            torch.cuda.synchronize(keep.device)
            ptr, n = keep.data_ptr(), pts.shape[0]
        out = np.empty(_abi.ALIGN_WORDS, np.float64)
        self._check(fn(self._ctx, C.c_void_p(ptr), int(n), _d3(T), float(min_weight), _d3(out)),
                    "align_terms")
        del keep
        return out[:36].reshape(6, 6).copy(), out[36:42].copy(), float(out[42]), int(out[43])

    def set_profiling(self, on=True):
        self._check(self._lib.tsdf_set_profiling(self._ctx, 1 if on else 0), "set_profiling")

    def set_profiling_period(self, every=_abi.KERNEL_KINDS, period=1):
        """Time the kinds in `every` on every batch, the others on every period-th batch."""
        mask = sum(1 << _abi.KERNEL_KINDS.index(k) for k in every)
        self._check(self._lib.tsdf_set_profiling_period(self._ctx, mask, int(period)),
                    "set_profiling_period")

    def set_metrics_log(self, path):
        """One JSON line per finished GPU batch appended to `path` (None: stop)."""
        self._check(self._lib.tsdf_set_metrics_log(
            self._ctx, None if path is None else str(path).encode()), "set_metrics_log")


class TsdfIntegratorConfig:
    """voxblox TsdfIntegratorBase::Config (the fields this backend implements; defaults as
    upstream, use_const_weight = False: 1 / z^2 of the point's sensor-frame depth, the sensor axis
    from T_G_C)."""

    def __init__(self, default_truncation_distance=0.1, max_weight=10000.0,
                 voxel_carving_enabled=True, min_ray_length_m=0.1, max_ray_length_m=5.0,
                 use_const_weight=False, allow_clear=True, use_weight_dropoff=True):
        self.default_truncation_distance = default_truncation_distance
        self.max_weight = max_weight
        self.voxel_carving_enabled = voxel_carving_enabled
        self.min_ray_length_m = min_ray_length_m
        self.max_ray_length_m = max_ray_length_m
        self.use_const_weight = use_const_weight
        self.allow_clear = allow_clear
        self.use_weight_dropoff = use_weight_dropoff


class SimpleTsdfIntegrator:
    """voxblox-named facade over a `semantics="voxblox"` volume (MAP_BACKEND_IDX 2's fusion rule
    on the GPU): `integratePointCloud(T_G_C, points_C)` transforms the sensor-frame points by the
    4x4 pose (float64, then float32) and integrates them from the pose's translation."""

    METHOD = "simple"

    def __init__(self, config, voxel_size, volume_cls=None, **kw):
        cls = volume_cls or HipTSDFVolume
        self.config = config
        self.volume = cls(voxel_size, config.default_truncation_distance,
                          space_carving=config.voxel_carving_enabled,
                          min_range=config.min_ray_length_m, max_range=config.max_ray_length_m,
                          semantics="voxblox", allow_clear=config.allow_clear,
                          use_weight_dropoff=config.use_weight_dropoff,
                          max_weight=config.max_weight, use_const_weight=config.use_const_weight,
                          method=self.METHOD, **kw)

    def integratePointCloud(self, T_G_C, points_C, colors=None, freespace_points=False):  # noqa: N802
        if freespace_points:
            raise NotImplementedError("freespace_points is not supported")
        T = np.asarray(T_G_C, np.float64).reshape(4, 4)
        pc = np.asarray(points_C, np.float64).reshape(-1, 3)
        pts_g = (pc @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        self.volume.integrate(pts_g, T)


class MergedTsdfIntegrator(SimpleTsdfIntegrator):
    """voxblox's MergedTsdfIntegrator (voxblox_ros's default `method`): the
    scan's points bundled per voxel, one weighted ray per bundle (tsdf_params.voxblox_method)."""

    METHOD = "merged"


def sector_ids(points, origin, n_sectors, yaw0=0.0):
    """The azimuth sector of every point (include/tsdf_hip.h tsdf_sector_of), in numpy fp32: the
    pseudo-angle of (x - ox, y - oy) against the sector starts.  -1 for NaN points."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    o = _origin_of(origin)
    if n_sectors <= 1:
        return np.where(np.isnan(pts[:, :2]).any(1), -1, 0)
    dx = pts[:, 0] - np.float32(o[0])
    dy = pts[:, 1] - np.float32(o[1])
    a = pseudo_angle(dx, dy)
    starts = np.array([pseudo_angle(np.float32(math.cos(t)), np.float32(math.sin(t)))
                       for t in (yaw0 + 2 * math.pi * k / n_sectors for k in range(n_sectors))],
                      np.float32)
    sec = np.full(pts.shape[0], -1, np.int64)
    for k in range(n_sectors):
        lo, hi = starts[k], starts[(k + 1) % n_sectors]
        m = (a >= lo) & (a < hi) if hi > lo else (a >= lo) | (a < hi)
        sec[m] = k
    return sec


def pseudo_angle(x, y):
    """fp32 pseudo-angle in [0, 4) (monotone in atan2), the sector rule's azimuth."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = x + y
        q1 = np.where(d > 0, y / np.where(d > 0, d, np.float32(1)), np.float32(0))
        q2 = np.float32(1) - x / (y - x)
        q3 = np.float32(2) - y / (-x - y)
        q4 = np.float32(3) + x / (x - y)
    return np.where(y >= 0, np.where(x >= 0, q1, q2), np.where(x < 0, q3, q4)).astype(np.float32)


def select_sector(points, origin, sector, n_sectors, yaw0=0.0):
    """Azimuth-sector shard of a scan (multi-GPU partitioning), via the library's C routine."""
    lib = load_hip_library()
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    o = _origin_of(origin)
    out = np.empty_like(pts)
    n = C.c_uint64()
    rc = lib.tsdf_select_sector(pts.ctypes.data_as(_abi.FP), pts.shape[0], _d3(o), float(yaw0),
                                int(sector), int(n_sectors), out.ctypes.data_as(_abi.FP),
                                C.byref(n))
    if rc != _abi.TSDF_OK:
        raise TsdfError(rc, "select_sector")
    return out[:n.value]
