"""The restatement the GPU deskew is held to (tests/deskewref.py), checked on its own: against the
fixed-pose restatement of tests/test_ouster.py when every column has the same pose; on a moving
platform, where it must put a ground plane and a wall back where they are; and the segment rule of
tsdf_map.ouster.frame_segments.  CPU suite."""
import numpy as np
import pytest

import deskewref as D
import ouster_ref as R
import ousterpkt

H, W, CPP = 16, 64, 16
PROFILE = "RNG19_RFL8_SIG16_NIR16"


def lut(h=H, w=W):
    from tsdf_map.scan_gen import make_xyz_lut
    meta = D.synthetic_meta(PROFILE, h, w, CPP)
    return make_xyz_lut(w, h, meta["lidar_origin_to_beam_origin_mm"], meta["beam_altitude_angles"],
                        meta["beam_azimuth_angles"])


def test_equal_column_poses_give_the_fixed_pose_points():
    fid, m_id, status, ts, px = ousterpkt.random_frame(PROFILE, H, W, CPP, 3)
    px[::5, ::3, :4] = 0                                   # some zero ranges
    status[[7, 30]] = 0
    packets = ousterpkt.write_frame(PROFILE, H, W, CPP, fid, m_id, status, ts, px)
    d, o = lut()
    c, s = np.cos(0.3), np.sin(0.3)
    P = np.array([[c, -s, 0.0, 3.25], [s, c, 0.0, -1.5], [0.0, 0.0, 1.0, 0.8]])
    xyz, r_cm = D.deskew_ref(packets, PROFILE, H, W, CPP, d, o, np.repeat(P[None], W, 0))
    rng = R.decode_frames(packets, PROFILE, H, W, CPP)[0]["RANGE"]
    assert np.array_equal(r_cm, rng.T) and not r_cm[[7, 30]].any()
    # tests/test_ouster.py:113-117: r dir + off, then ((m0 x + m1 y) + m2 z) + m3
    q = R.cartesian_f32(rng, d.astype(np.float32), o.astype(np.float32))
    m = P.astype(np.float32)
    want = np.stack([m[i, 0] * q[:, 0] + m[i, 1] * q[:, 1] + m[i, 2] * q[:, 2] + m[i, 3]
                     for i in range(3)], 1).astype(np.float32)
    got = xyz.reshape(W, H, 3).transpose(1, 0, 2).reshape(-1, 3)   # row-major
    nz = rng.reshape(-1) != 0
    assert 0 < np.count_nonzero(~nz) < nz.size
    assert np.array_equal(got[nz].view(np.uint32), want[nz].view(np.uint32))
    assert np.isnan(got[~nz]).all() and not np.isnan(got[nz]).any()


def test_moving_wall_is_put_back():
    """5 m/s and 0.5 rad/s over a 100 ms sweep: each column's ranges are cast from that column's
    true pose; the deskewed points lie on their planes within 2 mm (0.5 mm of range quantisation
    plus fp32 rounding, below 1e-5 m at these magnitudes), while the same ranges under the single
    mid-sweep pose miss them by more than 0.1 m somewhere (the scene has skew)."""
    from tsdf_map.ouster import OusterFormat, column_headers, column_poses
    fmt = OusterFormat(D.synthetic_meta(PROFILE, H, W, CPP))
    t0 = 10 ** 9
    ts = np.uint64(t0) + np.arange(W, dtype=np.uint64) * np.uint64(10 ** 8 // W)
    track = D.moving_track(t0 - 10 ** 7, t0 + 12 * 10 ** 7)
    mats, pose7 = column_poses(track, ts, np.ones(W, np.uint32))
    assert np.isfinite(mats).all() and np.isfinite(pose7).all()
    assert abs(mats[-1, 0, 3] - mats[0, 0, 3] - 5.0 * 0.1 * (W - 1) / W) < 1e-9
    d, o = lut()
    rng, plane = D.wall_frame(d, o, mats, H, W)
    assert rng.max() <= 60000 and np.count_nonzero(plane == 0) > 100 and \
        np.count_nonzero(plane == 1) > 100
    packets = ousterpkt.write_frame(PROFILE, H, W, CPP, 77, np.arange(W), np.ones(W), ts,
                                    D.range_pixels(rng))
    # the packets carry what the poses were built from
    hts, hst, hmid = column_headers(packets, fmt)
    assert np.array_equal(hts, ts) and np.array_equal(hmid, np.arange(W))
    mats2, _ = column_poses(track, hts, hst)
    assert np.array_equal(mats2, mats)
    xyz, r_cm = D.deskew_ref(packets, PROFILE, H, W, CPP, d, o, mats)
    assert np.array_equal(r_cm, rng)
    hit = plane.reshape(-1) >= 0
    assert np.array_equal(~np.isnan(xyz[:, 0]), hit)
    dist = D.plane_distance(xyz, plane.reshape(-1))
    print("deskewed: max plane distance %.3e m over %d points" % (np.nanmax(dist), hit.sum()))
    assert np.nanmax(dist) < 2e-3
    # the same ranges under one pose for the whole frame: skewed
    one, _ = D.deskew_ref(packets, PROFILE, H, W, CPP, d, o, np.repeat(mats[W // 2][None], W, 0))
    skew = D.plane_distance(one, plane.reshape(-1))
    print("single pose: max plane distance %.3f m" % np.nanmax(skew))
    assert np.nanmax(skew) > 0.1


def test_column_poses_mark_invalid_and_uncovered_columns():
    from tsdf_map.ouster import column_poses
    t0 = 10 ** 9
    ts = np.uint64(t0) + np.arange(W, dtype=np.uint64) * np.uint64(10 ** 8 // W)
    st = np.ones(W, np.uint32)
    st[5] = 0
    st[6] = 2                                               # bit 0 clear
    track = D.moving_track(t0, t0 + 5 * 10 ** 7)           # ends mid-sweep
    mats, pose7 = column_poses(track, ts, st)
    covered = (ts <= np.uint64(t0 + 5 * 10 ** 7)) & ((st & 1) != 0)
    assert np.array_equal(np.isfinite(mats).all(axis=(1, 2)), covered)
    assert np.array_equal(np.isnan(mats).all(axis=(1, 2)), ~covered)
    assert np.array_equal(np.isfinite(pose7).all(axis=1), covered)
    # the matrix is the quaternion's rotation and the position, in double
    v = 20
    p, q = track.at(int(ts[v]))
    yaw = 2 * np.arctan2(q[2], q[3])
    assert np.allclose(mats[v, :, :3], [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0],
                                        [0, 0, 1]], atol=1e-15)
    assert np.array_equal(mats[v, :, 3], p) and np.array_equal(pose7[v], np.concatenate([p, q]))
    # the time offset shifts the query; a gap wider than max_gap_ms has no pose
    m2, _ = column_poses(track, ts, st, time_offset_ns=-10 ** 7)
    assert np.isnan(m2[0]).all()                            # now before the track
    assert np.isnan(mats[35]).all() and np.isfinite(m2[35]).all()  # 54.7 ms -> 44.7 ms: covered
    m3, _ = column_poses(track, ts, st, max_gap_ms=5.0)
    assert np.isnan(m3[1]).all() and np.isfinite(m3[0]).all()  # column 0 sits on a track stamp


def _pose7(w, missing=()):
    p = np.arange(w * 7, dtype=np.float64).reshape(w, 7) + 1.0
    p[list(missing)] = np.nan
    return p


@pytest.mark.parametrize("K", [1, 7, W])
def test_segment_rule(K):
    from tsdf_map.ouster import frame_segments
    p7 = _pose7(W)
    offs, poses = frame_segments(p7, H, K)
    roffs, rposes = D.segments_ref(p7, H, K)
    assert offs.dtype == np.uint64 and offs.shape == (K + 1,) and poses.shape == (K, 7)
    assert np.array_equal(offs, roffs) and np.array_equal(poses, rposes)
    assert offs[0] == 0 and offs[-1] == H * W and np.all(np.diff(offs.astype(np.int64)) > 0)
    assert [int(x) for x in offs] == [H * (k * W // K) for k in range(K + 1)]
    if K == 1:
        assert np.array_equal(poses[0], p7[W // 2])
    if K == W:
        assert np.array_equal(poses, p7)
    if K == 7:  # does not divide w: segments of 9 and 10 columns
        assert sorted(set(np.diff(offs.astype(np.int64)) // H)) == [9, 10]


def test_segment_rule_without_poses_and_ties():
    from tsdf_map.ouster import frame_segments
    # K = 4: segments [0, 16), [16, 32), [32, 48), [48, 64), middles 8, 24, 40, 56
    missing = list(range(16, 32)) + [8] + [40, 41]
    p7 = _pose7(W, missing)
    p7[45, 2] = np.inf                                     # not finite: no pose either
    offs, poses = frame_segments(p7, H, 4)
    roffs, rposes = D.segments_ref(p7, H, 4)
    assert np.array_equal(offs, roffs) and np.array_equal(poses, rposes)
    assert np.array_equal(poses[0], p7[7])                 # 7 and 9 tie around 8: the lower
    assert np.array_equal(poses[1], [0, 0, 0, 0, 0, 0, 1])  # no pose in the segment
    assert np.array_equal(poses[2], p7[39])                # 39 is nearer 40 than 42
    assert np.array_equal(poses[3], p7[56])
    # a pose outside the segment is never taken
    lone = _pose7(W, range(1, W))
    _, poses = frame_segments(lone, H, 4)
    assert np.array_equal(poses[0], lone[0]) and np.array_equal(poses[1:, :6], np.zeros((3, 6)))
    for K in (0, W + 1, -1):
        with pytest.raises(ValueError):
            frame_segments(p7, H, K)
