"""2.5-D grids on top of `TSDFVolume.column_map` (include/tsdf_hip_columns.h): the column maps of a
box as one object, what a nav_msgs/OccupancyGrid holds, headroom and step height, and the
robot-centred call."""
import math

import numpy as np

from . import _abi
from .esdf import box_around


class ColumnMap:
    """The column maps of voxels lo..hi-1: elev, ceil (float32, metres, NaN where the column has
    no such surface), n_occ, n_free (uint16) and flags (uint8, COLUMN_* of tsdf_map._abi) as
    [y, x] arrays."""

    def __init__(self, elev, ceil, n_occ, n_free, flags, lo, hi, voxel_size):
        self.elev = np.asarray(elev, np.float32)
        self.ceil = np.asarray(ceil, np.float32)
        self.n_occ = np.asarray(n_occ, np.uint16)
        self.n_free = np.asarray(n_free, np.uint16)
        self.flags = np.asarray(flags, np.uint8)
        self.lo = np.asarray(lo, np.int64).reshape(3)
        self.hi = np.asarray(hi, np.int64).reshape(3)
        self.voxel_size = float(voxel_size)
        shape = (int(self.hi[1] - self.lo[1]), int(self.hi[0] - self.lo[0]))
        for a in (self.elev, self.ceil, self.n_occ, self.n_free, self.flags):
            if a.shape != shape:
                raise ValueError("every map must be a [y, x] array of the box's %r cells" % (shape,))

    @property
    def origin_xy(self):
        """World (x, y) of the corner of cell [0, 0]: lo[:2] * voxel_size."""
        return self.lo[:2].astype(np.float64) * self.voxel_size

    @property
    def resolution(self):
        return self.voxel_size

    def occupancy_grid(self, unknown=-1, free=0, occupied=100):
        """(data, origin_xy, resolution): data is int8 [y, x], row-major as
        nav_msgs/OccupancyGrid.data wants it (`occupied` where the column is OCCUPIED, `free`
        where it is FREE, `unknown` elsewhere), origin_xy = lo[:2] * voxel_size is the grid's
        info.origin.position and resolution = voxel_size its info.resolution."""
        data = np.full(self.flags.shape, unknown, np.int8)
        data[(self.flags & _abi.COLUMN_FREE) != 0] = free
        data[(self.flags & _abi.COLUMN_OCCUPIED) != 0] = occupied
        return data, self.origin_xy, self.resolution

    def headroom(self):
        """ceil - elev where the column has both, NaN elsewhere (negative under a shelf: the
        lowest underside lies below the highest top)."""
        both = _abi.COLUMN_HAS_ELEV | _abi.COLUMN_HAS_CEIL
        with np.errstate(invalid="ignore"):
            d = self.ceil - self.elev
        return np.where((self.flags & both) == both, d, np.float32(np.nan)).astype(np.float32)

    def step_height(self):
        """The largest |elev - elev of a 4-neighbour| per cell, over the neighbours that have an
        elevation; NaN where the cell has none or no such neighbour."""
        e = self.elev
        best = np.full(e.shape, np.nan, np.float32)
        for axis in (0, 1):
            if e.shape[axis] < 2:
                continue
            a = [slice(None)] * 2
            b = [slice(None)] * 2
            a[axis], b[axis] = slice(0, -1), slice(1, None)
            a, b = tuple(a), tuple(b)
            with np.errstate(invalid="ignore"):
                d = np.abs(e[b] - e[a])  # NaN where either side has no elevation
            best[a] = np.fmax(best[a], d)
            best[b] = np.fmax(best[b], d)
        return best


def columns_around(volume, center, half_extent_xy, z_min, z_max, **kw):
    """The column maps of the box of half-extent `half_extent_xy` (a number or (hx, hy), metres)
    around `center` in x, y and of the heights z_min..z_max (world metres) in z: the slab a robot
    of that height sweeps.  kw: `column_map`'s occ_band, min_weight, min_occ, min_free."""
    hxy = np.broadcast_to(np.asarray(half_extent_xy, np.float64), (2,))
    z_min, z_max = float(z_min), float(z_max)
    if not z_max >= z_min:
        raise ValueError("z_max < z_min")
    lo, hi = box_around(center, [hxy[0], hxy[1], 0.0], volume.voxel_size)
    # the voxels holding z_min .. z_max, by box_around's rule
    lo[2] = math.floor(z_min / volume.voxel_size)
    hi[2] = math.floor(z_max / volume.voxel_size) + 1
    return volume.column_map(lo, hi, **kw)
