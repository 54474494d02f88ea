"""Motion-compensated Ouster frames (include/tsdf_hip_deskew.h) restated in numpy -- test helper.

`headers_ref`   the column headers under the ScanBatcher rule (what tsdf_os_headers returns),
`deskew_ref`    k_os_deskew in fp32: column-major points, NaN where nothing is written,
`segments_ref`  the segment rule of tsdf_map.ouster.frame_segments, in plain loops,
and the moving platform the tests share: `moving_track` (5 m/s, 0.5 rad/s yaw, poses at 100 Hz),
`synthetic_meta` (sensor metadata of any size and profile) and `wall_frame` (ranges of a ground
plane and a wall seen from a pose per column).
"""
import math

import numpy as np

import ouster_ref as R
import ousterpkt


def headers_ref(packets, profile, h, w, columns_per_packet):
    """(timestamp uint64[w], status uint32[w], measurement_id uint16[w]): zero, then every valid
    column (m_id < w, status bit 0 set) of every packet, in order, at its m_id."""
    ts, st, mid = np.zeros(w, np.uint64), np.zeros(w, np.uint32), np.zeros(w, np.uint16)
    if not packets:
        return ts, st, mid
    _, m_id, status, stamp, _ = ousterpkt.read_columns(packets, profile, h, columns_per_packet)
    for m, s, t in zip(m_id.tolist(), status.tolist(), stamp.tolist()):
        if m >= w or not s & 1:
            continue
        ts[m], st[m], mid[m] = t, s, m
    return ts, st, mid


def column_major(lut, h, w):
    """A row-major (h*w, 3) LUT (index u w + v) as column-major (index v h + u), float32."""
    a = np.asarray(lut).astype(np.float32).reshape(h, w, 3)
    return np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(w * h, 3)


def pose_rows(x, y, z, m):
    """((m0 x + m1 y) + m2 z) + m3 per row, fp32; m: (n, 12) float32, one row per point."""
    return np.stack([((m[:, 4 * i] * x + m[:, 4 * i + 1] * y) + m[:, 4 * i + 2] * z)
                     + m[:, 4 * i + 3] for i in range(3)], 1).astype(np.float32)


def deskew_ref(packets, profile, h, w, columns_per_packet, lut_dir, lut_off, col_pose):
    """(xyz (w*h, 3) float32 column-major, range (w, h) uint32) of one frame's packets: RANGE as
    ouster_ref decodes it (missing and invalid columns are 0), rf = (float)r, x = rf dir + off,
    then the column's pose; NaN where r == 0.  lut_dir / lut_off: row-major (h*w, 3), as
    make_xyz_lut gives them; col_pose: (w, 3, 4) or (w, 12), rounded to float32 here."""
    rng = np.zeros((h, w), np.uint32)
    if packets:
        scans = R.decode_frames(packets, profile, h, w, columns_per_packet)
        assert len(scans) == 1, "one frame per call"
        rng = scans[0]["RANGE"].astype(np.uint32)
    r_cm = np.ascontiguousarray(rng.T)                       # (w, h)
    rf = r_cm.reshape(-1).astype(np.float32)
    d, o = column_major(lut_dir, h, w), column_major(lut_off, h, w)
    x, y, z = (rf * d[:, a] + o[:, a] for a in range(3))      # fp32 product, then fp32 sum
    m = np.asarray(col_pose, np.float64).reshape(w, -1)[:, :12].astype(np.float32)
    with np.errstate(invalid="ignore"):
        xyz = pose_rows(x, y, z, np.repeat(m, h, axis=0))
    xyz[rf == 0] = np.nan
    return xyz, r_cm


def segments_ref(col_pose7, h, K):
    """(scan_offsets, poses) by the segment rule, in plain loops."""
    p7 = np.asarray(col_pose7, np.float64)
    w = p7.shape[0]
    b = [k * w // K for k in range(K + 1)]
    poses = []
    for k in range(K):
        mid, best = (b[k] + b[k + 1]) // 2, None
        for v in range(b[k], b[k + 1]):
            if np.all(np.isfinite(p7[v])) and (best is None or abs(v - mid) < abs(best - mid)):
                best = v
        poses.append(p7[best] if best is not None else np.array([0, 0, 0, 0, 0, 0, 1.0]))
    return np.array([h * x for x in b], np.uint64), np.array(poses)


def moving_track(t0_ns, t1_ns, speed=5.0, yaw_rate=0.5, start=(3.25, -1.5, 1.5), yaw0=0.3,
                 step_ns=10 ** 7):
    """A PoseTrack of the sensor at 100 Hz over [t0_ns, t1_ns]: `speed` m/s along world x,
    yawing at `yaw_rate` rad/s about z."""
    from tsdf_map.ingest import PoseTrack
    track = PoseTrack()
    t = int(t0_ns)
    while True:
        t = min(t, int(t1_ns))
        s = (t - int(t0_ns)) * 1e-9
        yaw = yaw0 + yaw_rate * s
        track.add(t, [start[0] + speed * s, start[1], start[2]],
                  [0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2)])
        if t >= int(t1_ns):
            return track
        t += step_ns


def synthetic_meta(profile, h, w, columns_per_packet):
    """Sensor metadata (what OusterFormat reads) of an h x w sensor: beams from -22 to +12 degrees."""
    df = {"pixels_per_column": h, "columns_per_frame": w, "columns_per_packet": columns_per_packet}
    if profile != "LEGACY":
        df["udp_profile_lidar"] = profile
    return {"data_format": df,
            "beam_altitude_angles": np.linspace(12.0, -22.0, h).tolist(),
            "beam_azimuth_angles": (np.arange(h) % 4 * 1.4 - 2.1).tolist(),
            "lidar_origin_to_beam_origin_mm": 15.806}


WALL_PLANES = ((np.array([0.0, 0.0, 1.0]), 0.0),   # the ground, z = 0
               (np.array([1.0, 0.0, 0.0]), 20.0))  # a wall, x = 20


def wall_frame(lut_dir, lut_off, col_mats, h, w, max_range_m=55.0):
    """Ranges (mm, whole; 0 = no return) and the plane hit, both (w, h), of WALL_PLANES seen along
    the LUT's rays (row-major (h*w, 3), metres per mm and metres) from column v's pose
    col_mats[v] (3x4): the nearest positive intersection within max_range_m, in double."""
    d = np.asarray(lut_dir, np.float64).reshape(h, w, 3)
    o = np.asarray(lut_off, np.float64).reshape(h, w, 3)
    rng, plane = np.zeros((w, h), np.uint32), np.full((w, h), -1)
    for v in range(w):
        rot, t = col_mats[v][:, :3], col_mats[v][:, 3]
        dw, ow = d[:, v] @ rot.T, o[:, v] @ rot.T + t        # (h, 3) world
        best = np.full(h, np.inf)
        for k, (n, c) in enumerate(WALL_PLANES):
            den = dw @ n
            with np.errstate(divide="ignore", invalid="ignore"):
                r = (c - ow @ n) / den                       # mm along the ray
            ok = np.isfinite(r) & (r > 100.0) & (r < max_range_m * 1000.0) & (r < best)
            best[ok] = r[ok]
            plane[v, ok] = k
        hit = np.isfinite(best)
        rng[v, hit] = np.rint(best[hit]).astype(np.uint32)
    return rng, plane


def range_pixels(rng_cm, pixel_bytes=12):
    """(w, h, pixel_bytes) raw pixel bytes holding the (w, h) ranges at bytes 0..3 (RNG19 / LEGACY)."""
    px = np.zeros(rng_cm.shape + (pixel_bytes,), np.uint8)
    for k in range(4):
        px[..., k] = (rng_cm >> (8 * k)) & 0xFF
    return px


def plane_distance(xyz, plane):
    """|n . X - c| of every point to the plane it hit; NaN where it hit none.  xyz (n, 3), plane (n,)."""
    out = np.full(xyz.shape[0], np.nan)
    for k, (n, c) in enumerate(WALL_PLANES):
        sel = plane == k
        out[sel] = np.abs(xyz[sel].astype(np.float64) @ n - c)
    return out
