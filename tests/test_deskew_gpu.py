"""Motion-compensated Ouster frames on the GPU (include/tsdf_hip_deskew.h): k_os_deskew against the
numpy restatement (tests/deskewref.py) bit for bit on degraded synthetic frames of every profile,
and a recorded frame integrated as K sub-scans from a moving platform against the oracle."""
import glob
import json
import os

import numpy as np
import pytest

import deskewref as D
import oracle
import ouster_ref as R
import ousterpkt
from conftest import GOLDEN

W, CPP = 64, 16
PROFILES = list(R.PROFILES)
FRAME = [f for f in glob.glob(os.path.join(GOLDEN, "ouster", "*[0-9].json")) if "OS-2-128" in f][0]


@pytest.fixture(scope="module")
def small_volume():
    from tsdf_map import HipTSDFVolume
    with HipTSDFVolume(0.05, 0.15, max_points=1 << 12, max_bricks=1 << 10) as vol:
        yield vol


def degraded_frame(profile, h, seed):
    """Packets of one frame with random pixel bytes, status-0 columns, an id >= w and forced zero
    ranges, shuffled, one packet dropped; and a random pose per column with one NaN row."""
    rng = np.random.default_rng(seed)
    fid, m_id, status, ts, px = ousterpkt.random_frame(profile, h, W, CPP, seed)
    status[[4, 33]] = 0
    status[50] = 0xFFFE                                     # every bit but the valid one
    m_id[40] = W + 3
    px[rng.random((W, h)) < 0.1, :4] = 0                    # r == 0 (RANGE lies in bytes 0..3)
    packets = ousterpkt.write_frame(profile, h, W, CPP, fid, m_id, status, ts, px, pad=rng)
    packets = [packets[i] for i in (2, 0, 3)]               # shuffled; packet 1 dropped
    pose = rng.normal(0.0, 2.0, (W, 3, 4))
    pose[9] = np.nan
    return packets, pose


@pytest.mark.gpu
@pytest.mark.parametrize("h", [8, 33, 130])
@pytest.mark.parametrize("profile", PROFILES)
def test_kernel_bits(small_volume, profile, h):
    from tsdf_map.ouster import OusterFrontend
    fe = OusterFrontend(small_volume, D.synthetic_meta(profile, h, W, CPP))
    packets, pose = degraded_frame(profile, h, 100 + h)
    xyz, rng = fe.deskewed_points(packets, pose, with_range=True)
    fe.sync()
    g, gr = xyz.cpu().numpy(), rng.cpu().numpy().view(np.uint32)
    d, o = fe.lut_dir.cpu().numpy(), fe.lut_off.cpu().numpy()
    want, wr = D.deskew_ref(packets, profile, h, W, CPP, d, o, pose)
    ref = R.decode_frames(packets, profile, h, W, CPP)[0]["RANGE"]
    assert np.array_equal(gr, ref.T.astype(np.uint32)) and np.array_equal(gr, wr)
    # the frame has what it is meant to test
    assert not gr[[4, 33, 50, 40]].any() and not gr[CPP:2 * CPP].any() and gr[9].any()
    kept = np.setdiff1d(np.arange(W), [4, 33, 50, 40] + list(range(CPP, 2 * CPP)))
    assert gr[kept].any(axis=1).all() and (gr[kept] == 0).any() and gr.max() >= 1 << 14
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(g), nan)
    assert np.isnan(g[9 * h: 10 * h]).all() and not np.isnan(g).all()
    assert np.array_equal(nan.all(axis=1), nan.any(axis=1))  # whole triples
    assert np.array_equal(g.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.gpu
def test_degenerate_calls(small_volume):
    import ctypes as C

    from tsdf_map import _abi
    from tsdf_map.ouster import OusterFrontend
    h = 33
    fe = OusterFrontend(small_volume, D.synthetic_meta(PROFILES[1], h, W, CPP))
    pose = np.zeros((W, 3, 4))
    xyz, rng = fe.deskewed_points([], pose, with_range=True)   # no packets: the fill alone
    packets, pose = degraded_frame(PROFILES[1], h, 5)
    both, _ = fe.deskewed_points(packets, pose, with_range=True)
    only = fe.deskewed_points(packets, pose)                    # d_range_cm = NULL
    fe.sync()
    assert np.isnan(xyz.cpu().numpy()).all() and not rng.cpu().numpy().any()
    a, b = both.cpu().numpy().view(np.uint32), only.cpu().numpy().view(np.uint32)
    assert np.array_equal(a, b) and not np.isnan(only.cpu().numpy()).all()
    # argument rules: a NULL required buffer, too many columns
    lib, ctx = small_volume._lib, small_volume._ctx
    p = C.c_void_p(only.data_ptr())
    assert lib.tsdf_os_deskew_device(ctx, C.byref(fe.fmt.c), None, 0, p, p, p, None,
                                     None) == _abi.TSDF_EINVAL
    assert lib.tsdf_os_deskew_device(ctx, C.byref(fe.fmt.c), None, 1, p, p, p, p,
                                     None) == _abi.TSDF_EINVAL
    assert lib.tsdf_os_deskew_device(ctx, C.byref(fe.fmt.c), p, (1 << 16) + 1, p, p, p, p,
                                     None) == _abi.TSDF_EINVAL
    with pytest.raises(ValueError):
        fe.deskewed_points(packets, pose[:-1])


# ---- a recorded frame from a moving platform ---------------------------------------------------
def _frontend(meta):
    from tsdf_map import HipTSDFVolume
    from tsdf_map.ouster import OusterFrontend
    vol = HipTSDFVolume(0.05, 0.15, max_points=1 << 18, max_bricks=1 << 18, min_range=1e-3)
    return vol, OusterFrontend(vol, meta)


@pytest.fixture(scope="module")
def recorded():
    """The OS-2-128 frame, the moving track over its sweep (it ends 1 ms early: the last columns
    have no pose) and the restated points, computed once."""
    from tsdf_map.ouster import OusterFormat, column_headers, column_poses, read_pcap, split_frames
    from tsdf_map.scan_gen import make_xyz_lut
    meta = json.load(open(FRAME))
    fmt = OusterFormat(meta)
    size = R.layout(fmt.profile_name, fmt.h, fmt.columns_per_packet)[5]
    (fid, pk), = split_frames(read_pcap(FRAME.replace(".json", ".pcap"), fmt.port), fmt, size)
    ts, st, mid = column_headers(pk, fmt)
    valid = (st & 1) != 0
    t0, t1 = int(ts[valid].min()), int(ts[valid].max())
    track = D.moving_track(t0, t1 - 10 ** 6)
    mats, pose7 = column_poses(track, ts, st)
    d, o = make_xyz_lut(fmt.w, fmt.h, fmt.beam_origin_mm, fmt.altitude, fmt.azimuth)
    xyz, _ = D.deskew_ref(pk, fmt.profile_name, fmt.h, fmt.w, fmt.columns_per_packet, d, o, mats)
    return dict(meta=meta, fmt=fmt, packets=pk, track=track, pose7=pose7, xyz=xyz, valid=valid,
                span=(t0, t1))


def same_field(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [16, 7])
def test_recorded_frame_field_bitwise(recorded, K):
    """integrate_frame_deskewed == the oracle integrating each segment's restated points (NaN rows
    included) from that segment's position."""
    vol, fe = _frontend(recorded["meta"])
    xyz, info = fe.integrate_frame_deskewed(recorded["packets"], recorded["track"], segments=K)
    fe.sync()
    h, w = fe.fmt.h, fe.fmt.w
    offs, poses = D.segments_ref(recorded["pose7"], h, K)
    no_pose = int((recorded["valid"] & np.isnan(recorded["pose7"][:, 0])).sum())
    assert info == {"valid_columns": int(recorded["valid"].sum()), "columns_without_pose": no_pose,
                    "segments": K}
    assert 0 < no_pose < w // K                              # the track ends inside the last segment
    g, want = xyz.cpu().numpy(), recorded["xyz"]
    nan = np.isnan(want)
    assert nan[-h:].all() and np.array_equal(np.isnan(g), nan)
    assert np.array_equal(g.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    o = oracle.OracleTSDFVolume(0.05, 0.15, min_range=1e-3)
    for k in range(K):
        o.integrate(want[int(offs[k]): int(offs[k + 1])], poses[k, :3])
    field = vol.export_voxels()
    assert field[0].shape[0] > 10000
    same_field(field, o.export_voxels())
    assert vol.stats()["n_scans"] == K
    vol.close()


@pytest.mark.gpu
def test_constant_pose_equals_integrate_frame(recorded):
    """A platform at rest, one segment: the field of integrate_frame for the same pose, bit for
    bit (there an r = 0 pixel is the sensor origin, which min_range drops; here it is NaN)."""
    from tsdf_map.ingest import PoseTrack
    from tsdf_map.ouster import column_poses
    t0, t1 = recorded["span"]
    p, q = [3.25, -1.5, 0.8], [0.0, 0.0, np.sin(0.65), np.cos(0.65)]
    track = PoseTrack()
    track.add(t0 - 10 ** 6, p, q)
    track.add(t1 + 10 ** 6, p, q)
    mats, _ = column_poses(track, np.arange(t0, t1, 10 ** 6), np.ones(1 + (t1 - t0) // 10 ** 6),
                           max_gap_ms=1e3)
    assert (mats == mats[0]).all()                          # at rest: one pose, whatever the stamp
    P = np.vstack([mats[0], [0.0, 0.0, 0.0, 1.0]])
    a, fa = _frontend(recorded["meta"])
    xyz, info = fa.integrate_frame_deskewed(recorded["packets"], track, segments=1, max_gap_ms=1e3)
    fa.sync()
    assert info["columns_without_pose"] == 0 and info["segments"] == 1
    b, fb = _frontend(recorded["meta"])
    imgs, pts = fb.integrate_frame(recorded["packets"], P)
    fb.sync()
    # the points too, wherever there is one: column-major here, row-major there
    h, w = fa.fmt.h, fa.fmt.w
    g = xyz.cpu().numpy().reshape(w, h, 3).transpose(1, 0, 2).reshape(-1, 3)
    nz = imgs["RANGE"].cpu().numpy().reshape(-1) != 0
    assert np.array_equal(g[nz].view(np.uint32), pts.cpu().numpy()[nz].view(np.uint32))
    assert np.isnan(g[~nz]).all()
    field = a.export_voxels()
    assert field[0].shape[0] > 10000
    same_field(field, b.export_voxels())
    assert a.stats()["n_scans"] == 1
    a.close()
    b.close()
