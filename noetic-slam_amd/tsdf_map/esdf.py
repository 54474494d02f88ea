"""Robot-centred distance fields on top of `TSDFVolume.esdf` (include/tsdf_hip_esdf.h): the box
around a point, the field as a grid that answers clearance queries, and the padded call that makes
the clearances exact at the box's rim."""
import numpy as np

from . import _abi


def box_around(center, half_extent_m, voxel_size):
    """The voxel box (lo, hi), hi exclusive, of the world-frame box of centre `center` and
    half-extent(s) `half_extent_m` (a number or one per axis):
    lo = floor((c - h) / vs), hi = floor((c + h) / vs) + 1 in double."""
    c = np.asarray(center, np.float64).reshape(3)
    h = np.broadcast_to(np.asarray(half_extent_m, np.float64), (3,))
    vs = float(voxel_size)
    lo = np.floor((c - h) / vs).astype(np.int64)
    hi = np.floor((c + h) / vs).astype(np.int64) + 1
    return lo, hi


class EsdfGrid:
    """A distance field of voxels lo..lo + shape - 1: dist and flags as [z, y, x] arrays."""

    def __init__(self, dist, flags, lo, voxel_size):
        self.dist = np.asarray(dist, np.float32)
        self.flags = np.asarray(flags, np.uint8)
        if self.dist.ndim != 3 or self.flags.shape != self.dist.shape:
            raise ValueError("dist and flags must be [z, y, x] arrays of one shape")
        self.lo = np.asarray(lo, np.int64).reshape(3)
        self.voxel_size = float(voxel_size)

    @property
    def hi(self):
        return self.lo + np.array(self.dist.shape[::-1], np.int64)

    def _index(self, points):
        """(inside (n,), z, y, x) of the voxels holding world points (n, 3)."""
        p = np.asarray(points, np.float64).reshape(-1, 3)
        with np.errstate(invalid="ignore"):
            v = np.floor(p / self.voxel_size)
            inside = np.all(np.isfinite(v) & (v >= self.lo) & (v < self.hi), axis=1)
        ijk = np.where(inside[:, None], v, self.lo).astype(np.int64) - self.lo
        return inside, ijk[:, 2], ijk[:, 1], ijk[:, 0]

    def clearance(self, points):
        """dist of the voxel holding each point (nearest voxel, no interpolation); NaN outside the
        box."""
        inside, z, y, x = self._index(points)
        return np.where(inside, self.dist[z, y, x], np.float32(np.nan)).astype(np.float32)

    def known(self, points):
        """True where the point's voxel is observed (False outside the box)."""
        inside, z, y, x = self._index(points)
        return inside & ((self.flags[z, y, x] & _abi.ESDF_OBSERVED) != 0)

    def gradient(self):
        """Central differences of dist in metres per metre, [z, y, x, 3] with components (x, y, z);
        one-sided at the box's faces, 0 along an axis of one voxel."""
        g = np.zeros(self.dist.shape + (3,), np.float32)
        d = self.dist.astype(np.float64)
        for comp, axis in ((0, 2), (1, 1), (2, 0)):
            if d.shape[axis] > 1:
                g[..., comp] = np.gradient(d, self.voxel_size, axis=axis)
        return g


def esdf_around(volume, center, half_extent_m, max_dist, pad=True, site_band=None, min_weight=0.0):
    """The distance field of the box around `center` as an EsdfGrid.  pad: compute the box grown by
    radius_vox on every side and crop, so that every clearance below max_dist is exact with
    respect to the whole map, not only to the surface inside the box."""
    lo, hi = box_around(center, half_extent_m, volume.voxel_size)
    r = volume.esdf_radius(max_dist) if pad else 0
    dist, flags = volume.esdf(lo - r, hi + r, max_dist, site_band=site_band, min_weight=min_weight)
    if r:
        dist = np.ascontiguousarray(dist[r:-r, r:-r, r:-r])
        flags = np.ascontiguousarray(flags[r:-r, r:-r, r:-r])
    return EsdfGrid(dist, flags, lo, volume.voxel_size)

