"""The indexed mesh on the host side: a PLY writer and piecewise meshing of a large or windowed map
(TSDFVolume.extract_indexed_mesh; include/tsdf_hip_mesh.h)."""
import itertools
import os

import numpy as np


def write_ply(path, vertices, triangles, normals=None):
    """A binary little-endian PLY of (vertices (V, 3) float32, triangles (T, 3) indices, normals
    (V, 3) float32 or None).  Written to a temporary file beside `path` and renamed over it, so a
    reader never sees half a file."""
    v = np.ascontiguousarray(vertices, "<f4").reshape(-1, 3)
    t = np.ascontiguousarray(triangles).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= v.shape[0]):
        raise ValueError("triangle index out of range")
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0],
            "property float x", "property float y", "property float z"]
    if normals is not None:
        n = np.ascontiguousarray(normals, "<f4").reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError("normals must match vertices")
        head += ["property float nx", "property float ny", "property float nz"]
        v = np.concatenate([v, n], axis=1)
    head += ["element face %d" % t.shape[0], "property list uchar uint vertex_indices",
             "end_header"]
    faces = np.empty(t.shape[0], np.dtype([("n", "u1"), ("i", "<u4", (3,))]))
    faces["n"] = 3
    faces["i"] = t
    tmp = "%s.tmp.%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            f.write(("\n".join(head) + "\n").encode("ascii"))
            f.write(np.ascontiguousarray(v).tobytes())
            f.write(faces.tobytes())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def tile_boxes(brick_coords, tile_voxels):
    """The boxes [lo, hi) of the voxel-aligned grid of `tile_voxels` (an int or three) that hold a
    voxel of one of the bricks, as a list of (lo, hi) int64[3] pairs in (z, y, x) order."""
    tv = np.broadcast_to(np.asarray(tile_voxels, np.int64), (3,))
    if np.any(tv < 1):
        raise ValueError("tile_voxels must be positive")
    b = np.asarray(brick_coords, np.int64).reshape(-1, 3)
    first = (8 * b) // tv          # floor division: the grid is aligned at voxel 0
    last = (8 * b + 7) // tv
    tiles = set()
    for f, l in zip(first, last):
        tiles.update(itertools.product(*(range(int(f[a]), int(l[a]) + 1) for a in range(3))))
    out = []
    for t in sorted(tiles, key=lambda t: (t[2], t[1], t[0])):
        lo = np.asarray(t, np.int64) * tv
        out.append((lo, lo + tv))
    return out


def mesh_tiles(volume, tile_voxels, **kw):
    """Mesh a map piece by piece: yields (lo, hi, (vertices, triangles, normals)) for every box of
    the voxel-aligned `tile_voxels` grid that the map's bricks touch, in (z, y, x) order; **kw goes
    to `extract_indexed_mesh`.  Every cube is meshed in exactly one box (the box of its min voxel),
    so the pieces' triangles together are the whole mesh; vertices on a box face appear in both
    neighbours.  A sliding-window user re-meshes only the boxes that changed."""
    for lo, hi in tile_boxes(volume.brick_coords(), tile_voxels):
        yield lo, hi, volume.extract_indexed_mesh(lo=lo, hi=hi, **kw)
