"""Levels of detail (include/tsdf_hip_coarsen.h): a map and its 2:1 reductions, each level on the
GPU at twice the voxel size and about an eighth of the memory of the one before -- what
`mesh_tiles`, `esdf` and `column_map` read instead of the sensor-resolution map over a large box.
"""


def lod_pyramid(volume, levels, **kw):
    """[volume, level 1, ..., level `levels`]: level k is `coarsened(**kw)` of level k - 1
    (min_children, min_weight as `HipTSDFVolume.coarsened` takes them), so its voxel size is
    2^k times the volume's.  `volume` is not changed; the new volumes are closed again if a level
    fails."""
    if int(levels) < 0:
        raise ValueError("levels must be >= 0")
    volume._coarsen_fn("tsdf_coarsen_into")  # a library that cannot coarsen says so here
    out = [volume]
    try:
        for _ in range(int(levels)):
            out.append(out[-1].coarsened(**kw))
    except Exception:
        for v in out[1:]:
            v.close()
        raise
    return out
