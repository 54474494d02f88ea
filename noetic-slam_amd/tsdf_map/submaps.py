"""Fusing submaps (include/tsdf_hip_merge.h): short local volumes, each anchored at its own pose,
merged into one global volume at their optimised poses -- the pieces a `SlidingWindow` or an
archive leaves behind, the poses a pose-graph back end or `align.refine_pose` produces.
"""


def fuse_submaps(volumes, poses, into=None, **kw):
    """Merge every volume of `volumes` at its pose (T_global_submap, (3, 4) or (4, 4)) into one
    volume, in order: `into`, or a new empty volume with the first submap's parameters.  **kw goes
    to `TSDFVolume.merge_from` (mode, min_weight).  Returns (volume, [counts per merge]).  The
    submaps are not changed; a volume created here is closed again if a merge fails."""
    volumes = list(volumes)
    poses = list(poses)
    if len(volumes) != len(poses):
        raise ValueError("%d volumes but %d poses" % (len(volumes), len(poses)))
    if into is None and not volumes:
        raise ValueError("no submap and no volume to fuse into")
    for v in volumes:
        v._merge_fn("tsdf_merge_transformed")  # a library that cannot merge says so here
    out = volumes[0].empty_like() if into is None else into
    counts = []
    try:
        for v, T in zip(volumes, poses):
            counts.append(out.merge_from(v, T, **kw))
    except Exception:
        if into is None:
            out.close()
        raise
    return out, counts
