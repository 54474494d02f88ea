"""Range images of the map: a spinning lidar's ray pattern and `TSDFVolume.raycast` behind it.

The rays are in the sensor frame; the pose given to `range_image` places them in the world, so one
ray table serves every pose (the model scan of scan-to-model registration, a predicted range image
to compare with a live scan, a depth view of the map without meshing it).
"""
import math

import numpy as np


def spherical_rays(h, w, elev_lo, elev_hi):
    """(h * w, 3) float32 unit directions of an h-beam, w-column spinning sensor, column-major in
    firing order: all h beams of column 0, then column 1, ...  Beam u looks at elevation
    elev_lo + u (elev_hi - elev_lo) / (h - 1) (radians; h = 1: elev_lo), column v at azimuth
    -2 pi v / w (the encoder turns clockwise seen from above, as an Ouster's does); x forward,
    z up."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("h and w must be positive")
    u = np.arange(h, dtype=np.float64)
    elev = elev_lo + u * ((elev_hi - elev_lo) / (h - 1)) if h > 1 else np.full(1, float(elev_lo))
    az = -2.0 * math.pi * np.arange(w, dtype=np.float64) / w
    ce = np.cos(elev)[None, :]
    d = np.stack([np.cos(az)[:, None] * ce, np.sin(az)[:, None] * ce,
                  np.broadcast_to(np.sin(elev)[None, :], (w, h))], -1)  # [column][beam]
    return np.ascontiguousarray(d.reshape(-1, 3).astype(np.float32))


def range_image(vol, pose, rays, shape=None, **kw):
    """The map seen from `pose` (3x4 or 4x4, world from sensor) along `rays` (sensor-frame
    directions from the sensor's origin, e.g. `spherical_rays`): (depth, hit) images.  shape =
    (h, w) for column-major rays of h beams and w columns gives h x w images (row = beam); without
    it the images are flat.  Further keywords go to `TSDFVolume.raycast` (t_min, t_max, step,
    mode, min_weight)."""
    rays = np.asarray(rays, np.float32)
    depth, _, hit = vol.raycast(np.zeros(3, np.float32), rays, pose=pose, normals=False, **kw)
    if shape is not None:
        h, w = shape
        if h * w != depth.shape[0]:
            raise ValueError("shape does not match the number of rays")
        depth = np.ascontiguousarray(depth.reshape(w, h).T)
        hit = np.ascontiguousarray(hit.reshape(w, h).T)
    return depth, hit
