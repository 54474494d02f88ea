"""Frontier voxels on top of `TSDFVolume.frontiers` (include/tsdf_hip_frontier.h): the set as one
object with world points and directions, its runs per brick, its connected clusters (what a
frontier-based exploration planner ranks) and the robot-centred call."""
import numpy as np

from .esdf import box_around

# the 13 offsets (dx, dy, dz) of 26-connectivity that come later in (z, y, x) order
_HALF_26 = [(dx, dy, dz) for dz in (0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) > (0, 0, 0)]


class FrontierCluster:
    """One connected component of a `FrontierSet`: `indices` into the set (ascending), `size`,
    `centroid` (world metres), `mean_direction` (the unit sum of the voxels' dir, zero where it
    cancels) and the voxel bounds `lo` / `hi` (hi exclusive)."""

    def __init__(self, indices, coords, dirs, voxel_size):
        self.indices = indices
        self.size = int(indices.shape[0])
        c = coords[indices].astype(np.float64)
        self.centroid = (c.mean(axis=0) + 0.5) * voxel_size
        d = dirs[indices].astype(np.int64).sum(axis=0).astype(np.float64)
        n = float(np.sqrt((d * d).sum()))
        self.mean_direction = d / n if n > 0 else np.zeros(3)
        self.lo = coords[indices].min(axis=0).astype(np.int64)
        self.hi = coords[indices].max(axis=0).astype(np.int64) + 1


class FrontierSet:
    """The frontier voxels of a box: coords (N, 3) int32 voxel indices, n_unknown (N,) uint8 (the
    unknown voxels among each one's neighbourhood), dir (N, 3) int8 (the sum of the offsets to
    them), counts (tsdf_frontier_counts as a dict) and the voxel size.  Ordered by brick in
    (z, y, x) order, then by in-brick voxel."""

    def __init__(self, coords, n_unknown, dir, counts, voxel_size):  # noqa: A002
        self.coords = np.asarray(coords, np.int32).reshape(-1, 3)
        self.n_unknown = np.asarray(n_unknown, np.uint8).reshape(-1)
        self.dir = np.asarray(dir, np.int8).reshape(-1, 3)
        n = self.coords.shape[0]
        if self.n_unknown.shape[0] != n or self.dir.shape[0] != n:
            raise ValueError("coords, n_unknown and dir must hold one row per frontier voxel")
        self.counts = dict(counts)
        self.voxel_size = float(voxel_size)

    def __len__(self):
        return self.coords.shape[0]

    @property
    def points(self):
        """World centres (N, 3) float64: (coords + 0.5) * voxel_size."""
        return (self.coords.astype(np.float64) + 0.5) * self.voxel_size

    @property
    def directions(self):
        """dir at unit length (N, 3) float64; zero where dir is (0, 0, 0)."""
        d = self.dir.astype(np.float64)
        n = np.sqrt((d * d).sum(axis=1, keepdims=True))
        return np.divide(d, n, out=np.zeros_like(d), where=n > 0)

    def brick_runs(self):
        """(bricks (B, 3) int32, start (B,), length (B,)): the set's voxels of brick b are rows
        start[b] .. start[b] + length[b] - 1; bricks in (z, y, x) order, as the set is."""
        n = len(self)
        if n == 0:
            return np.zeros((0, 3), np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64)
        b = self.coords >> 3
        first = np.ones(n, bool)
        first[1:] = np.any(b[1:] != b[:-1], axis=1)
        start = np.flatnonzero(first).astype(np.int64)
        length = np.diff(np.append(start, n)).astype(np.int64)
        return b[start].astype(np.int32), start, length

    def clusters(self, min_voxels=1):
        """The connected components of the set under 26-connectivity with at least `min_voxels`
        voxels, as `FrontierCluster`s: largest first, equal sizes by their smallest voxel in
        (z, y, x) order.  Host numpy: a union-find over the sorted linear keys."""
        n = len(self)
        if n == 0:
            return []
        c = self.coords.astype(np.int64)
        lo = c.min(axis=0) - 1
        ext = c.max(axis=0) + 2 - lo  # one spare cell per side: an offset never wraps
        key = ((c[:, 2] - lo[2]) * ext[1] + (c[:, 1] - lo[1])) * ext[0] + (c[:, 0] - lo[0])
        order = np.argsort(key, kind="stable")
        skey = key[order]
        ea, eb = [], []
        for dx, dy, dz in _HALF_26:
            want = skey + ((dz * ext[1] + dy) * ext[0] + dx)
            j = np.searchsorted(skey, want)
            hit = j < n
            hit[hit] = skey[j[hit]] == want[hit]
            ea.append(np.flatnonzero(hit))
            eb.append(j[hit])
        ea, eb = np.concatenate(ea), np.concatenate(eb)
        # labels[i] <= i names a voxel of i's component (positions in key order); at the fixed
        # point every component carries its smallest position
        labels = np.arange(n)
        while True:
            la, lb = labels[ea], labels[eb]
            m = np.minimum(la, lb)
            new = labels.copy()
            for t in (la, lb, ea, eb):
                np.minimum.at(new, t, m)
            while True:
                nn = new[new]
                if np.array_equal(nn, new):
                    break
                new = nn
            if np.array_equal(new, labels):
                break
            labels = new
        roots, inv, sizes = np.unique(labels, return_inverse=True, return_counts=True)
        members = np.argsort(inv, kind="stable")  # positions in key order, grouped by component
        first = np.cumsum(sizes) - sizes
        out = []
        # (roots ascend: the smallest voxel of a component in (z, y, x) order)
        for r in np.lexsort((roots, -sizes)):
            if sizes[r] < min_voxels:
                continue
            idx = np.sort(order[members[first[r]:first[r] + sizes[r]]])
            out.append(FrontierCluster(idx, self.coords, self.dir, self.voxel_size))
        return out


def frontiers_around(volume, center, half_extent, **kw):
    """The frontier voxels of the box of half-extent `half_extent` (a number or one per axis,
    metres) around `center` (world metres).  kw: `frontiers`' free_band, min_weight, connectivity,
    min_unknown."""
    lo, hi = box_around(center, half_extent, volume.voxel_size)
    return volume.frontiers(lo, hi, **kw)
