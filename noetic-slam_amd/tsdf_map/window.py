"""A bounded live map: the bricks around the sensor stay on the GPU, the rest goes to an archive.

`SlidingWindow` wraps a volume that can evict (include/tsdf_hip_prune.h): every few scans it
removes the bricks outside a cube around the scan origin and appends them, in `export_bricks`'
format, to an archive -- host memory or `.npz` parts on disk.  A brick that leaves, is seen again
and leaves again is in the archive twice, one copy per generation (one `append` is one generation,
and holds each brick at most once); `full_map()` merges the generations and the live bricks
through `import_bricks`, whose weighted mean of two copies is the sum the unevicted map would
hold (exact in the weights; the distances agree to the rounding of the mean).

With `coarse` (a volume of twice the voxel size, include/tsdf_hip_coarsen.h) every eviction first
fuses the 2:1 reduction of the leaving bricks into it, on the GPU: the space outside the window
stays readable -- raycast, distance field, column maps -- at an eighth of the memory, without
re-importing the archive.  Coarsening disjoint sets of bricks one after the other equals
coarsening their union (rule 9 of the header), so the coarse map is exactly the coarsening of
everything that has left the window, as long as no brick leaves twice.  A brick that is seen
again and leaves again is fused a second time by the weighted mean, each generation's coarse value
standing for that generation's voxels: an approximation of coarsening the summed fine bricks
(DESIGN.md §24).
"""
import ctypes as C
import math
import os

import numpy as np

from . import _abi
from .volume import TsdfError, _origin_of


def cube_box(center, radius_m, voxel_size):
    """The brick box (lo, hi), lo <= b < hi, of the world-frame cube of half-side radius_m around
    center: lo = floor((c - r) / (8 vs)), hi = floor((c + r) / (8 vs)) + 1 per axis in float64,
    clamped to the packable brick coordinates (csrc/prune_plan.h states the same rule in C++)."""
    side = 8.0 * float(voxel_size)
    lo, hi = [], []
    for c in np.asarray(center, np.float64).reshape(3):
        a = _clamp(_floor_div(float(c) - float(radius_m), side))
        b = _clamp(_floor_div(float(c) + float(radius_m), side) + 1.0)
        lo.append(a)
        hi.append(max(a, b))
    return np.array(lo, np.int32), np.array(hi, np.int32)


def _floor_div(x, side):
    q = x / side  # (IEEE division; math.floor refuses inf and NaN, which clamp below)
    return math.floor(q) if math.isfinite(q) else q


def _clamp(b):
    if b != b:
        return 0
    return int(min(max(b, _abi.BRICK_COORD_MIN), _abi.BRICK_COORD_MAX))


class MemoryArchive:
    """Evicted bricks kept in host memory, one entry per generation."""

    def __init__(self):
        self.parts = []

    def append(self, coords, sdf, weight):
        if len(coords):
            self.parts.append((np.array(coords, np.int32), np.array(sdf, np.float32),
                               np.array(weight, np.float32)))

    def __len__(self):
        return len(self.parts)

    def __iter__(self):
        return iter(self.parts)

    def num_bricks(self):
        return sum(len(p[0]) for p in self.parts)


class NpzArchive:
    """Evicted bricks as numbered `.npz` parts in a directory, one part per generation; an
    existing directory's parts are kept and iterated first."""

    def __init__(self, directory, compressed=False):
        self.directory = str(directory)
        self.compressed = compressed
        os.makedirs(self.directory, exist_ok=True)
        self._n = len(self._names())

    def _names(self):
        return sorted(f for f in os.listdir(self.directory)
                      if f.startswith("part_") and f.endswith(".npz"))

    def append(self, coords, sdf, weight):
        if not len(coords):
            return
        save = np.savez_compressed if self.compressed else np.savez
        save(os.path.join(self.directory, "part_%06d.npz" % self._n),
             coords=np.asarray(coords, np.int32), sdf=np.asarray(sdf, np.float32),
             weight=np.asarray(weight, np.float32))
        self._n += 1

    def __len__(self):
        return self._n

    def __iter__(self):
        for name in self._names():
            with np.load(os.path.join(self.directory, name), allow_pickle=False) as z:
                yield z["coords"], z["sdf"], z["weight"]

    def num_bricks(self):
        return sum(len(p[0]) for p in self)


class SlidingWindow:
    """`volume` bounded to the cube of half-side radius_m around the latest scan origin: every
    `every` scans the bricks outside go to `archive` (anything with append(coords, sdf, weight);
    default a MemoryArchive).  coarse: a volume of twice the voxel size that takes the 2:1
    reduction of every brick that leaves, before it leaves (None: nothing of the kind)."""

    def __init__(self, volume, radius_m, every=8, archive=None, coarse=None):
        if not radius_m >= 0:
            raise ValueError("radius_m must be >= 0")
        if int(every) < 1:
            raise ValueError("every must be >= 1")
        volume._prune_fn("tsdf_evict_outside")  # a volume that cannot evict says so here
        if coarse is not None:
            coarse._coarsen_fn("tsdf_coarsen_into")
            if np.float32(coarse.voxel_size) != np.float32(2.0) * np.float32(volume.voxel_size):
                raise ValueError("coarse must have twice the volume's voxel size (%g against %g)"
                                 % (coarse.voxel_size, volume.voxel_size))
        self.coarse = coarse
        self.volume = volume
        self.radius_m = float(radius_m)
        self.every = int(every)
        self.archive = MemoryArchive() if archive is None else archive
        self.n_scans = 0
        self.n_evicted = 0

    def integrate(self, points, extrinsic):
        self.volume.integrate(points, extrinsic)
        self.n_scans += 1
        if self.n_scans % self.every == 0:
            self.evict(_origin_of(extrinsic))

    def evict(self, center):
        """Evict outside the cube around `center` now; returns the bricks archived."""
        lo, hi = cube_box(center, self.radius_m, self.volume.voxel_size)
        if self.coarse is not None:
            self.coarse.coarsen_from(self.volume, box=(lo, hi), side="outside")
        coords, sdf, weight = self.volume.evict_outside(lo, hi)
        self.archive.append(coords, sdf, weight)
        self.n_evicted += len(coords)
        return len(coords)

    def full_map(self, volume=None):
        """A volume holding the archive and the live bricks: `volume` (empty, same parameters),
        or a new one of the live volume's class and parameters.  One generation per import, since
        an import wants each brick once; the live map is not changed."""
        v = self.volume
        if volume is None:
            p = v.params
            volume = type(v).__new__(type(v))
            volume._lib = v._lib
            volume._ctx = C.c_void_p()
            q = _abi.TsdfParams.from_buffer_copy(p)
            rc = v._lib.tsdf_create(C.byref(q), C.byref(volume._ctx))
            if rc != _abi.TSDF_OK:
                volume._ctx = C.c_void_p()
                raise TsdfError(rc, "tsdf_create failed (full_map)")
            volume._adopt(q)
            if hasattr(v, "tensor_device"):
                volume.tensor_device = v.tensor_device
        for coords, sdf, weight in self.archive:
            volume.import_bricks(coords, sdf, weight)
        volume.import_bricks(*v.export_bricks())
        return volume
